// Sliding-window stereo bundle adjustment (include/sship.h "Window smoother"): the objective of WindowSmoother::optimize
// (stereo reprojection under isotropic Huber-robust noise, slot 0 fixed) with the landmarks as variables eliminated by the Schur
// complement and the pose-only solver's Levenberg-Marquardt schedule.
//   k_ba_solve   one 256-thread workgroup per window, the whole LM loop inside the launch; the grid is min(windows, kBaResident)
//                workgroups that walk the windows, each with a workspace slice of its own, so a window sees nothing of the others.
//     setup      obs_of[l][k] = the lowest present row of landmark l in slot k (atomicMin); activity, the initial points and the list of
//                active landmarks in ascending l (one wave, ballot compaction).
//     linearise  one thread per active landmark: C_l, c_l and the W_kl blocks (global workspace);  then per slot k >= 1 the 27 sums of
//                A_k and a_k: per thread over its rows in index order, a lane butterfly, the waves in order.
//     trial      one thread per active landmark: the 3x3 Cholesky C_l + lambda I = L L^T, Z_kl = W_kl L^-T, v_l = L^-1 c_l;  then every
//                entry of S (lower triangle) and b has ONE owner thread, which walks the active landmarks in ascending l, three FMAs per
//                entry and landmark seen by both slots (S_kk' -= Z_kl Z_k'l^T keeps S symmetric by construction; a thread owns whole rows
//                of 6x6 blocks, and the landmarks' masks and rows are staged in LDS 128 at a time);  S lives in LDS and is factorised
//                there column by column by the whole workgroup;  forward and back substitution likewise;  the poses (se3_retract,
//                solver_math.h) and the landmarks move;  the cost at the candidate is one more pass (all threads over all rows,
//                butterfly, waves).
//                Every thread carries the scalars of the schedule (lambda, c, trials) itself, from values broadcast through LDS, so every
//                branch of the loop is uniform.
//   k_ba_tracks  one workgroup per window, slot after slot: the winning predecessor of a row by atomicMax in LDS.
// No local array is indexed by a run-time value; nothing lives in scratch: profiles/ba_solve_resource_usage.txt.
#include "../../include/sship.h"
#include "kernels.h"
#include "solver_math.h"

namespace sship {

namespace {

constexpr int kBaThreads = 256;
constexpr int kBaNone = 0x7fffffff;
constexpr int kBaTile = 128;

// One observation of point X from pose T (row-major [R | t], any address space): the whitened residual and rho; false behind the camera.
struct BaRes { double x, y, z, iz, r0, r1, r2, w, rho; bool front; };
__device__ __forceinline__ BaRes ba_residual(const double* T, double X0, double X1, double X2, float uL, float uR, float v, const BaK& P) {
  BaRes o;
  const double d0 = X0 - T[3], d1 = X1 - T[7], d2 = X2 - T[11];
  o.x = T[0] * d0 + T[4] * d1 + T[8] * d2;
  o.y = T[1] * d0 + T[5] * d1 + T[9] * d2;
  o.z = T[2] * d0 + T[6] * d1 + T[10] * d2;
  o.front = o.z > 0.0;
  const double s = P.inv_sigma;
  if (!o.front) {
    o.iz = 0.0;
    o.r0 = o.r1 = o.r2 = 2.0 * P.fx * s;
  } else {
    o.iz = 1.0 / o.z;
    o.r0 = (P.fx * o.x * o.iz + P.cx - (double)uL) * s;
    o.r1 = (P.fx * (o.x - P.baseline) * o.iz + P.cx - (double)uR) * s;
    o.r2 = (P.fy * o.y * o.iz + P.cy - (double)v) * s;
  }
  const double e2 = o.r0 * o.r0 + o.r1 * o.r1 + o.r2 * o.r2;
  const double e = sqrt(e2);
  const bool quad = e <= P.k;
  o.w = quad ? 1.0 : P.k / e;
  o.rho = quad ? 0.5 * e2 : P.k * e - 0.5 * P.k2;
  return o;
}

// whitened gradients of the three residuals with respect to q: (a0, 0, a2) for uL, (a0, 0, c2) for uR, (0, b1, b2) for v
struct BaGrad { double a0, a2, c2, b1, b2; };
__device__ __forceinline__ BaGrad ba_grad(const BaRes& o, const BaK& P) {
  BaGrad g;
  const double fiz = P.fx * o.iz * P.inv_sigma, giz = P.fy * o.iz * P.inv_sigma;
  g.a0 = fiz; g.a2 = -fiz * o.x * o.iz; g.c2 = -fiz * (o.x - P.baseline) * o.iz;
  g.b1 = giz; g.b2 = -giz * o.y * o.iz;
  return g;
}

// the workspace slice of one resident workgroup (ba_workspace_bytes)
struct BaWs {
  double *X, *Xn, *Cl, *cl, *v, *Li, *W, *Z;
  int *obs_of, *lmask, *act, *amask;
};
__device__ __forceinline__ BaWs ba_slice(char* base, int K, int N, int L) {
  BaWs w;
  double* d = reinterpret_cast<double*>(base);
  w.X = d; d += 3 * (size_t)L;
  w.Xn = d; d += 3 * (size_t)L;
  w.Cl = d; d += 6 * (size_t)L;
  w.cl = d; d += 3 * (size_t)L;
  w.v = d; d += 3 * (size_t)L;
  w.Li = d; d += 6 * (size_t)L;
  w.W = d; d += 18 * (size_t)K * N;
  w.Z = d; d += 18 * (size_t)K * N;
  int* i = reinterpret_cast<int*>(d);
  w.obs_of = i; i += (size_t)L * K;
  w.lmask = i; i += L;
  w.act = i; i += L;
  w.amask = i;
  return w;
}

}  // namespace

size_t ba_workspace_bytes(int K, int N, int L) {
  const size_t b = (size_t)L * (4 * (size_t)K + 204) + 288 * (size_t)K * N;
  return (b + 15) / 16 * 16;
}

__global__ __launch_bounds__(kBaThreads) void k_ba_solve(const float* __restrict__ meas, const int32_t* __restrict__ track,
                                                        const int32_t* __restrict__ n_kf_dev, const double* __restrict__ pose0, int K, int N, int L,
                                                        int windows, BaK P, char* __restrict__ ws_base, size_t ws_stride,
                                                        double* __restrict__ pose, int32_t* __restrict__ stats, double* __restrict__ cost,
                                                        float* __restrict__ landmarks) {
  extern __shared__ double s_dyn[];               // S [6 (K - 1)][ld], then b [6 (K - 1)]
  __shared__ double s_T[kBaMaxKf * 12];           // the state's poses
  __shared__ double s_Tn[kBaMaxKf * 12];          // the candidate's
  __shared__ double s_A[(kBaMaxKf - 1) * 27];     // per slot k >= 1: A_k (21, upper triangle by rows), a_k (6)
  __shared__ double s_red[4][27];
  __shared__ double s_val;
  __shared__ int s_nobs, s_nact, s_flag;
  __shared__ int s_tmask[kBaTile], s_tl[kBaTile];           // a tile of active landmarks: slot masks, ids
  __shared__ unsigned short s_trow[kBaTile * kBaMaxKf];     //   and their row per slot
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_max = 6 * (K - 1), ld = n_max | 1;
  double* S = s_dyn;
  double* s_b = s_dyn + (size_t)n_max * ld;
  const BaWs ws = ba_slice(ws_base + (size_t)blockIdx.x * ws_stride, K, N, L);

  for (int win = blockIdx.x; win < windows; win += gridDim.x) {
    __syncthreads();  // the previous window's last readers of LDS
    const float* wm = meas + (size_t)win * K * N * 3;
    const int32_t* wt = track + (size_t)win * K * N;
    const double* wp0 = pose0 + (size_t)win * K * 12;
    double* wpose = pose + (size_t)win * K * 12;
    const int n_kf = n_kf_dev ? min(max(n_kf_dev[win], 0), K) : K;
    const int n = 6 * max(n_kf - 1, 0);

    // ---- setup: poses, the observation table, activity, initial points ----
    if (tid == 0) { s_nobs = 0; s_nact = 0; s_flag = 0; }
    __syncthreads();
    for (int i = tid; i < K * 12; i += kBaThreads) {
      const double t = wp0[i];
      s_T[i] = t; s_Tn[i] = t;
      if (i < n_kf * 12 && !solver_finite(t)) atomicOr(&s_flag, 1);
    }
    for (size_t i = tid; i < (size_t)L * K; i += kBaThreads) ws.obs_of[i] = kBaNone;
    __syncthreads();
    const bool bad_input = s_flag != 0;
    for (int k = 0; k < n_kf; ++k)
      for (int i = tid; i < N; i += kBaThreads) {
        const int t = wt[k * N + i];
        if ((unsigned)t >= (unsigned)L) continue;
        const float* m = wm + ((size_t)k * N + i) * 3;
        if (solver_finitef(m[0]) && solver_finitef(m[1]) && solver_finitef(m[2])) atomicMin(&ws.obs_of[(size_t)t * K + k], i);
      }
    __syncthreads();
    {
      int cnt = 0;
      for (int l = tid; l < L; l += kBaThreads) {
        int mask = 0, seen = 0, first = -1;
        for (int k = 0; k < n_kf; ++k) {
          const int row = ws.obs_of[(size_t)l * K + k];
          if (row == kBaNone) continue;
          mask |= 1 << k; ++seen;
          const float* m = wm + ((size_t)k * N + row) * 3;
          if (first < 0 && (double)m[0] - (double)m[1] > 0.0) first = k;
        }
        const bool active = seen >= 2 && first >= 0;
        ws.lmask[l] = active ? mask : 0;
        if (active) {
          cnt += seen;
          const float* m = wm + ((size_t)first * N + ws.obs_of[(size_t)l * K + first]) * 3;
          const double uL = m[0], uR = m[1], v = m[2];
          const double Zc = P.fx * P.baseline / (uL - uR);
          const double Xc = (uL - P.cx) * Zc / P.fx, Yc = (v - P.cy) * Zc / P.fy;
          const double* T = s_T + first * 12;
          ws.X[3 * (size_t)l + 0] = T[0] * Xc + T[1] * Yc + T[2] * Zc + T[3];
          ws.X[3 * (size_t)l + 1] = T[4] * Xc + T[5] * Yc + T[6] * Zc + T[7];
          ws.X[3 * (size_t)l + 2] = T[8] * Xc + T[9] * Yc + T[10] * Zc + T[11];
        }
      }
      if (cnt) atomicAdd(&s_nobs, cnt);
    }
    __syncthreads();
    if (wave == 0) {  // the active landmarks in ascending l
      int base = 0;
      for (int l0 = 0; l0 < L; l0 += 64) {
        const int l = l0 + lane;
        const int mask = l < L ? ws.lmask[l] : 0;
        const unsigned long long bal = __ballot(mask != 0);
        if (mask != 0) {
          const int j = base + __popcll(bal & ((1ull << lane) - 1ull));
          ws.act[j] = l; ws.amask[j] = mask;
        }
        base += __popcll(bal);
      }
      if (lane == 0) s_nact = base;
    }
    __syncthreads();
    const int n_obs = s_nobs, n_act = s_nact;
    int status = SSHIP_BA_CONVERGED, trials = 0;
    double c = 0.0, c_init = 0.0, lambda = P.lambda0;
    if (bad_input) status = SSHIP_BA_BAD_INPUT;
    else if (n_kf < 2 || n_act == 0) status = SSHIP_BA_TOO_FEW;
    const bool early = status != SSHIP_BA_CONVERGED;

    // the cost at (Ts, Xs): every thread over its rows of every slot in order, a butterfly, the waves in order -> returned to every thread
    auto cost_at = [&](const double* Ts, const double* Xs) -> double {
      double acc = 0.0;
      for (int k = 0; k < n_kf; ++k)
        for (int i = tid; i < N; i += kBaThreads) {
          const int t = wt[k * N + i];
          if ((unsigned)t >= (unsigned)L) continue;
          if (ws.lmask[t] == 0 || ws.obs_of[(size_t)t * K + k] != i) continue;
          const float* m = wm + ((size_t)k * N + i) * 3;
          acc += ba_residual(Ts + k * 12, Xs[3 * (size_t)t], Xs[3 * (size_t)t + 1], Xs[3 * (size_t)t + 2], m[0], m[1], m[2], P).rho;
        }
#pragma unroll
      for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 64);
      __syncthreads();  // s_red, s_val free
      if (lane == 0) s_red[wave][0] = acc;
      __syncthreads();
      if (tid == 0) s_val = ((s_red[0][0] + s_red[1][0]) + s_red[2][0]) + s_red[3][0];
      __syncthreads();
      return s_val;
    };

    // C_l, c_l, W_kl, A_k, a_k at the state (s_T, ws.X)
    auto linearise = [&]() {
      for (int j = tid; j < n_act; j += kBaThreads) {
        const int l = ws.act[j], mask = ws.amask[j];
        const double X0 = ws.X[3 * (size_t)l], X1 = ws.X[3 * (size_t)l + 1], X2 = ws.X[3 * (size_t)l + 2];
        double C00 = 0, C01 = 0, C02 = 0, C11 = 0, C12 = 0, C22 = 0, g0 = 0, g1 = 0, g2 = 0;
        for (int k = 0; k < n_kf; ++k) {
          if (!((mask >> k) & 1)) continue;
          const int row = ws.obs_of[(size_t)l * K + k];
          const float* m = wm + ((size_t)k * N + row) * 3;
          const double* T = s_T + k * 12;
          const BaRes o = ba_residual(T, X0, X1, X2, m[0], m[1], m[2], P);
          double Jl[3][3], Jp[3][6];
          if (o.front) {
            const BaGrad g = ba_grad(o, P);
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {  // rows of J_l = grad^T R^T
              Jl[0][cc] = g.a0 * T[4 * cc] + g.a2 * T[4 * cc + 2];
              Jl[1][cc] = g.a0 * T[4 * cc] + g.c2 * T[4 * cc + 2];
              Jl[2][cc] = g.b1 * T[4 * cc + 1] + g.b2 * T[4 * cc + 2];
            }
            Jp[0][0] = -g.a2 * o.y; Jp[0][1] = g.a2 * o.x - g.a0 * o.z; Jp[0][2] = g.a0 * o.y; Jp[0][3] = -g.a0; Jp[0][4] = 0.0; Jp[0][5] = -g.a2;
            Jp[1][0] = -g.c2 * o.y; Jp[1][1] = g.c2 * o.x - g.a0 * o.z; Jp[1][2] = g.a0 * o.y; Jp[1][3] = -g.a0; Jp[1][4] = 0.0; Jp[1][5] = -g.c2;
            Jp[2][0] = g.b1 * o.z - g.b2 * o.y; Jp[2][1] = g.b2 * o.x; Jp[2][2] = -g.b1 * o.x; Jp[2][3] = 0.0; Jp[2][4] = -g.b1; Jp[2][5] = -g.b2;
          } else {
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
              for (int cc = 0; cc < 3; ++cc) Jl[r][cc] = 0.0;
#pragma unroll
              for (int cc = 0; cc < 6; ++cc) Jp[r][cc] = 0.0;
            }
          }
          const double w = o.w;
          C00 += w * (Jl[0][0] * Jl[0][0] + Jl[1][0] * Jl[1][0] + Jl[2][0] * Jl[2][0]);
          C01 += w * (Jl[0][0] * Jl[0][1] + Jl[1][0] * Jl[1][1] + Jl[2][0] * Jl[2][1]);
          C02 += w * (Jl[0][0] * Jl[0][2] + Jl[1][0] * Jl[1][2] + Jl[2][0] * Jl[2][2]);
          C11 += w * (Jl[0][1] * Jl[0][1] + Jl[1][1] * Jl[1][1] + Jl[2][1] * Jl[2][1]);
          C12 += w * (Jl[0][1] * Jl[0][2] + Jl[1][1] * Jl[1][2] + Jl[2][1] * Jl[2][2]);
          C22 += w * (Jl[0][2] * Jl[0][2] + Jl[1][2] * Jl[1][2] + Jl[2][2] * Jl[2][2]);
          g0 += w * (Jl[0][0] * o.r0 + Jl[1][0] * o.r1 + Jl[2][0] * o.r2);
          g1 += w * (Jl[0][1] * o.r0 + Jl[1][1] * o.r1 + Jl[2][1] * o.r2);
          g2 += w * (Jl[0][2] * o.r0 + Jl[1][2] * o.r1 + Jl[2][2] * o.r2);
          if (k >= 1) {
            double* Wp = ws.W + ((size_t)k * N + row) * 18;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
              for (int cc = 0; cc < 3; ++cc) Wp[a * 3 + cc] = w * (Jp[0][a] * Jl[0][cc] + Jp[1][a] * Jl[1][cc] + Jp[2][a] * Jl[2][cc]);
          }
        }
        double* Cp = ws.Cl + 6 * (size_t)l;
        Cp[0] = C00; Cp[1] = C01; Cp[2] = C02; Cp[3] = C11; Cp[4] = C12; Cp[5] = C22;
        double* gp = ws.cl + 3 * (size_t)l;
        gp[0] = g0; gp[1] = g1; gp[2] = g2;
      }
      for (int k = 1; k < n_kf; ++k) {
        double acc[27];
#pragma unroll
        for (int i = 0; i < 27; ++i) acc[i] = 0.0;
        const double* T = s_T + k * 12;
        for (int i = tid; i < N; i += kBaThreads) {
          const int t = wt[k * N + i];
          if ((unsigned)t >= (unsigned)L) continue;
          if (ws.lmask[t] == 0 || ws.obs_of[(size_t)t * K + k] != i) continue;
          const float* m = wm + ((size_t)k * N + i) * 3;
          const BaRes o = ba_residual(T, ws.X[3 * (size_t)t], ws.X[3 * (size_t)t + 1], ws.X[3 * (size_t)t + 2], m[0], m[1], m[2], P);
          if (!o.front) continue;  // zero Jacobian
          const BaGrad g = ba_grad(o, P);
          const double J[3][6] = {{-g.a2 * o.y, g.a2 * o.x - g.a0 * o.z, g.a0 * o.y, -g.a0, 0.0, -g.a2},
                                  {-g.c2 * o.y, g.c2 * o.x - g.a0 * o.z, g.a0 * o.y, -g.a0, 0.0, -g.c2},
                                  {g.b1 * o.z - g.b2 * o.y, g.b2 * o.x, -g.b1 * o.x, 0.0, -g.b1, -g.b2}};
          int q = 0;
#pragma unroll
          for (int a = 0; a < 6; ++a) {
            const double wa0 = o.w * J[0][a], wa1 = o.w * J[1][a], wa2 = o.w * J[2][a];
#pragma unroll
            for (int b = a; b < 6; ++b) { acc[q] += wa0 * J[0][b] + wa1 * J[1][b] + wa2 * J[2][b]; ++q; }
            acc[21 + a] += wa0 * o.r0 + wa1 * o.r1 + wa2 * o.r2;
          }
        }
#pragma unroll
        for (int i = 0; i < 27; ++i) {
          double v = acc[i];
#pragma unroll
          for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
          acc[i] = v;
        }
        __syncthreads();  // s_red free
        if (lane == 0) {
#pragma unroll
          for (int i = 0; i < 27; ++i) s_red[wave][i] = acc[i];
        }
        __syncthreads();
        if (tid < 27) s_A[(k - 1) * 27 + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
      }
      __syncthreads();
    };

    if (!early) {
      linearise();
      c = cost_at(s_T, ws.X);
      c_init = c;
      for (;;) {
        if (trials >= P.max_iterations) { status = SSHIP_BA_ITER_CAP; break; }
        ++trials;
        // ---- the landmarks' 3x3 factors ----
        if (tid == 0) s_flag = 0;
        __syncthreads();
        {
          bool fail = false;
          for (int j = tid; j < n_act; j += kBaThreads) {
            const int l = ws.act[j], mask = ws.amask[j];
            const double* Cp = ws.Cl + 6 * (size_t)l;
            const double* gp = ws.cl + 3 * (size_t)l;
            const double d0 = Cp[0] + lambda;
            const double l00 = sqrt(d0), i00 = 1.0 / l00;
            const double l10 = Cp[1] * i00, l20 = Cp[2] * i00;
            const double d1 = Cp[3] + lambda - l10 * l10;
            const double l11 = sqrt(d1), i11 = 1.0 / l11;
            const double l21 = (Cp[4] - l20 * l10) * i11;
            const double d2 = Cp[5] + lambda - l20 * l20 - l21 * l21;
            const double l22 = sqrt(d2), i22 = 1.0 / l22;
            if (!(d0 > 0.0) || !(d1 > 0.0) || !(d2 > 0.0)) { fail = true; continue; }
            // L^-1 (lower): rows (i00), (i10, i11), (i20, i21, i22)
            const double i10 = -l10 * i00 * i11, i21 = -l21 * i11 * i22, i20 = -(l20 * i00 + l21 * i10) * i22;
            double* Lp = ws.Li + 6 * (size_t)l;
            Lp[0] = i00; Lp[1] = i10; Lp[2] = i11; Lp[3] = i20; Lp[4] = i21; Lp[5] = i22;
            double* vp = ws.v + 3 * (size_t)l;
            vp[0] = i00 * gp[0]; vp[1] = i10 * gp[0] + i11 * gp[1]; vp[2] = i20 * gp[0] + i21 * gp[1] + i22 * gp[2];
            for (int k = 1; k < n_kf; ++k) {
              if (!((mask >> k) & 1)) continue;
              const size_t o = ((size_t)k * N + ws.obs_of[(size_t)l * K + k]) * 18;
#pragma unroll
              for (int a = 0; a < 6; ++a) {  // Z = W L^-T
                const double w0 = ws.W[o + a * 3], w1 = ws.W[o + a * 3 + 1], w2 = ws.W[o + a * 3 + 2];
                ws.Z[o + a * 3] = w0 * i00;
                ws.Z[o + a * 3 + 1] = w0 * i10 + w1 * i11;
                ws.Z[o + a * 3 + 2] = w0 * i20 + w1 * i21 + w2 * i22;
              }
            }
          }
          if (fail) atomicOr(&s_flag, 1);
        }
        __syncthreads();
        bool ok = s_flag == 0;
        __syncthreads();  // s_flag is cleared again at the top of the next trial
        if (ok) {
          // ---- S (lower triangle) and b: one owner per entry, the active landmarks in ascending l ----
          // A task is one row a of one 6x6 block (kr, kc), kc <= kr: its six entries, and b's entry on a diagonal block.  At most 3 tasks per
          // thread (120 blocks x 6 rows at 16 keyframes).  The masks, ids and rows of kBaTile landmarks at a time are staged in LDS.
          const int n_tasks = (n_kf - 1) * n_kf / 2 * 6;
          double acc[3][7];
          int t_kr[3], t_kc[3], t_a[3];
#pragma unroll
          for (int u = 0; u < 3; ++u) {
#pragma unroll
            for (int q = 0; q < 7; ++q) acc[u][q] = 0.0;
            const int t = tid + u * kBaThreads;
            int kr = 1, kc = 1;
            if (t < n_tasks) {
              const int bi = t / 6;
              int r = 0;
              while ((r + 1) * (r + 2) / 2 <= bi) ++r;
              kr = r + 1; kc = bi - r * (r + 1) / 2 + 1;
            }
            t_kr[u] = kr; t_kc[u] = kc; t_a[u] = t % 6;
          }
          for (int base = 0; base < n_act; base += kBaTile) {
            const int cnt = min(kBaTile, n_act - base);
            __syncthreads();  // the previous tile's readers
            for (int j = tid; j < cnt; j += kBaThreads) { s_tmask[j] = ws.amask[base + j]; s_tl[j] = ws.act[base + j]; }
            for (int e = tid; e < cnt * K; e += kBaThreads) {
              const int row = ws.obs_of[(size_t)ws.act[base + e / K] * K + e % K];
              s_trow[e] = (unsigned short)(row == kBaNone ? 0 : row);
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 3; ++u) {
              if (tid + u * kBaThreads >= n_tasks) continue;
              const int kr = t_kr[u], kc = t_kc[u], a = t_a[u];
              for (int j = 0; j < cnt; ++j) {
                const int mask = s_tmask[j];
                if (!((mask >> kr) & (mask >> kc) & 1)) continue;
                const double* zr = ws.Z + ((size_t)kr * N + s_trow[j * K + kr]) * 18 + a * 3;
                const double* zc = ws.Z + ((size_t)kc * N + s_trow[j * K + kc]) * 18;
                const double z0 = zr[0], z1 = zr[1], z2 = zr[2];
#pragma unroll
                for (int b = 0; b < 6; ++b) acc[u][b] += z0 * zc[b * 3] + z1 * zc[b * 3 + 1] + z2 * zc[b * 3 + 2];
                if (kr == kc) {
                  const double* vp = ws.v + 3 * (size_t)s_tl[j];
                  acc[u][6] += z0 * vp[0] + z1 * vp[1] + z2 * vp[2];
                }
              }
            }
          }
#pragma unroll
          for (int u = 0; u < 3; ++u) {
            if (tid + u * kBaThreads >= n_tasks) continue;
            const int kr = t_kr[u], kc = t_kc[u], a = t_a[u];
            const int r = (kr - 1) * 6 + a;
            const double* Ak = s_A + (kr - 1) * 27;
#pragma unroll
            for (int b = 0; b < 6; ++b) {
              const int cc = (kc - 1) * 6 + b;
              if (cc > r) continue;
              double d = 0.0;
              if (kr == kc) {  // A_k[b][a], b <= a, out of the upper triangle by rows
                d = Ak[b * 6 - b * (b - 1) / 2 + (a - b)];
                if (a == b) d += lambda;
              }
              S[r * ld + cc] = d - acc[u][b];
            }
            if (kr == kc) s_b[r] = -Ak[21 + a] + acc[u][6];
          }
          __syncthreads();
          // ---- Cholesky of S in place (lower), right-looking, column by column ----
          for (int j = 0; j < n; ++j) {
            const double d = S[j * ld + j];
            if (!(d > 0.0)) { ok = false; break; }  // uniform: every thread read the same value
            const double lj = sqrt(d), il = 1.0 / lj;
            __syncthreads();
            if (tid == 0) S[j * ld + j] = lj;
            for (int i = j + 1 + tid; i < n; i += kBaThreads) S[i * ld + j] *= il;
            __syncthreads();
            const int m = n - j - 1;
            for (int e = tid; e < m * m; e += kBaThreads) {
              const int i = j + 1 + e / m, q = j + 1 + e % m;
              if (q <= i) S[i * ld + q] -= S[i * ld + j] * S[q * ld + j];
            }
            __syncthreads();
          }
        }
        if (ok) {
          // ---- L y = b, L^T delta = y, in place in s_b ----
          for (int j = 0; j < n; ++j) {
            __syncthreads();
            const double yj = s_b[j] / S[j * ld + j];
            __syncthreads();
            if (tid == 0) s_b[j] = yj;
            for (int i = j + 1 + tid; i < n; i += kBaThreads) s_b[i] -= S[i * ld + j] * yj;
          }
          for (int j = n - 1; j >= 0; --j) {
            __syncthreads();
            const double xj = s_b[j] / S[j * ld + j];
            __syncthreads();
            if (tid == 0) s_b[j] = xj;
            for (int i = tid; i < j; i += kBaThreads) s_b[i] -= S[j * ld + i] * xj;
          }
          __syncthreads();
          // ---- the candidate ----
          if (tid >= 1 && tid < n_kf) {
            double delta[6], Tl[12], Tn[12];
#pragma unroll
            for (int i = 0; i < 6; ++i) delta[i] = s_b[(tid - 1) * 6 + i];
#pragma unroll
            for (int i = 0; i < 12; ++i) Tl[i] = s_T[tid * 12 + i];
            se3_retract(Tl, delta, Tn);
#pragma unroll
            for (int i = 0; i < 12; ++i) s_Tn[tid * 12 + i] = Tn[i];
          }
          for (int j = tid; j < n_act; j += kBaThreads) {
            const int l = ws.act[j], mask = ws.amask[j];
            const double* vp = ws.v + 3 * (size_t)l;
            double t0 = vp[0], t1 = vp[1], t2 = vp[2];
            for (int k = 1; k < n_kf; ++k) {
              if (!((mask >> k) & 1)) continue;
              const double* z = ws.Z + ((size_t)k * N + ws.obs_of[(size_t)l * K + k]) * 18;
              const double* dk = s_b + (k - 1) * 6;
#pragma unroll
              for (int a = 0; a < 6; ++a) { t0 += z[a * 3] * dk[a]; t1 += z[a * 3 + 1] * dk[a]; t2 += z[a * 3 + 2] * dk[a]; }
            }
            const double* Lp = ws.Li + 6 * (size_t)l;  // delta_l = -L^-T t
            ws.Xn[3 * (size_t)l] = ws.X[3 * (size_t)l] - (Lp[0] * t0 + Lp[1] * t1 + Lp[3] * t2);
            ws.Xn[3 * (size_t)l + 1] = ws.X[3 * (size_t)l + 1] - (Lp[2] * t1 + Lp[4] * t2);
            ws.Xn[3 * (size_t)l + 2] = ws.X[3 * (size_t)l + 2] - Lp[5] * t2;
          }
          __syncthreads();
          const double cn = cost_at(s_Tn, ws.Xn);
          const bool conv = solver_finite(cn) && fabs(c - cn) <= fmax(P.abs_tol, P.rel_tol * c);
          if (conv || cn < c) {  // the candidate becomes the state
            for (int i = 12 + tid; i < n_kf * 12; i += kBaThreads) s_T[i] = s_Tn[i];
            for (int j = tid; j < n_act; j += kBaThreads) {
              const size_t l = (size_t)ws.act[j];
              ws.X[3 * l] = ws.Xn[3 * l]; ws.X[3 * l + 1] = ws.Xn[3 * l + 1]; ws.X[3 * l + 2] = ws.Xn[3 * l + 2];
            }
            c = cn;
            __syncthreads();
            if (conv) { status = SSHIP_BA_CONVERGED; break; }
            lambda /= 10.0;
            linearise();
            continue;
          }
        }
        lambda *= 10.0;
        if (lambda > P.lambda_max) { status = SSHIP_BA_STALLED; break; }
      }
    }

    // ---- outputs: every entry written ----
    __syncthreads();
    for (int i = tid; i < K * 12; i += kBaThreads) {
      const int k = i / 12;
      wpose[i] = (early || k == 0 || k >= n_kf) ? wp0[i] : s_T[i];
    }
    if (landmarks) {
      float* wl = landmarks + (size_t)win * L * 3;
      const float qnan = __int_as_float(0x7fc00000);
      for (int l = tid; l < L; l += kBaThreads) {
        const bool on = !early && ws.lmask[l] != 0;
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) wl[3 * (size_t)l + cc] = on ? (float)ws.X[3 * (size_t)l + cc] : qnan;
      }
    }
    if (tid == 0) {
      stats[win * 4 + 0] = n_obs; stats[win * 4 + 1] = n_act; stats[win * 4 + 2] = trials; stats[win * 4 + 3] = status;
      cost[win * 2 + 0] = early ? 0.0 : c_init; cost[win * 2 + 1] = early ? 0.0 : c;
    }
  }
}

// One workgroup per window, slot after slot; s_win[j] = the highest row i of slot k - 1 that matches row j and carries a track.
__global__ __launch_bounds__(256) void k_ba_tracks(const uint8_t* __restrict__ has_depth, const int32_t* __restrict__ matches,
                                                  const int32_t* __restrict__ n_dev, const int32_t* __restrict__ n_kf_dev, int K, int N,
                                                  int32_t* __restrict__ track) {
  __shared__ int s_win[kBaMaxObs];
  const int win = blockIdx.x, tid = threadIdx.x;
  const uint8_t* hd = has_depth + (size_t)win * K * N;
  const int32_t* mt = matches + (size_t)win * (K - 1) * N;
  int32_t* tr = track + (size_t)win * K * N;
  const int n_kf = n_kf_dev ? min(max(n_kf_dev[win], 0), K) : K;
  for (int k = 0; k < K; ++k) {
    if (k >= n_kf) {
      for (int j = tid; j < N; j += 256) tr[k * N + j] = -1;
      continue;
    }
    const int nk = min(max(n_dev[win * K + k], 0), N);
    if (k == 0) {
      for (int j = tid; j < N; j += 256) tr[j] = (j < nk && hd[j] != 0) ? j : -1;
    } else {
      const int np = min(max(n_dev[win * K + k - 1], 0), N);
      for (int j = tid; j < N; j += 256) s_win[j] = -1;
      __syncthreads();
      for (int i = tid; i < np; i += 256) {
        const int j = mt[(k - 1) * N + i];
        if ((unsigned)j < (unsigned)nk && tr[(k - 1) * N + i] >= 0) atomicMax(&s_win[j], i);
      }
      __syncthreads();
      for (int j = tid; j < N; j += 256) {
        int t = -1;
        if (j < nk && hd[k * N + j] != 0) t = s_win[j] >= 0 ? tr[(k - 1) * N + s_win[j]] : k * N + j;
        tr[k * N + j] = t;
      }
    }
    __syncthreads();  // slot k's tracks are read by slot k + 1
  }
}

int ba_solve_lds_bytes(int K) {
  const int n = 6 * (K - 1), ld = n | 1;
  return (n * ld + n) * (int)sizeof(double);
}

hipError_t ba_solve_prepare() {  // once per handle: more than 64 KB of dynamic LDS (16 keyframes) has to be asked for
  return hipFuncSetAttribute(reinterpret_cast<const void*>(k_ba_solve), hipFuncAttributeMaxDynamicSharedMemorySize, ba_solve_lds_bytes(kBaMaxKf));
}

void launch_ba_solve(const float* meas, const int32_t* track, const int32_t* n_kf, const double* pose0, int K, int N, int L, int windows,
                     const BaK& k, void* ws, double* pose, int32_t* stats, double* cost, float* landmarks, hipStream_t s) {
  const int grid = windows < kBaResident ? windows : kBaResident;
  hipLaunchKernelGGL(k_ba_solve, dim3(grid), dim3(kBaThreads), ba_solve_lds_bytes(K), s, meas, track, n_kf, pose0, K, N, L, windows, k,
                     static_cast<char*>(ws), ba_workspace_bytes(K, N, L), pose, stats, cost, landmarks);
}
void launch_ba_tracks(const uint8_t* has_depth, const int32_t* matches, const int32_t* n, const int32_t* n_kf, int K, int N, int windows,
                      int32_t* track, hipStream_t s) {
  hipLaunchKernelGGL(k_ba_tracks, dim3(windows), dim3(256), 0, s, has_depth, matches, n, n_kf, K, N, track);
}

}  // namespace sship
