// Device maths shared by the three solvers (pose_kernels.hip, ba_kernels.hip, pg_kernels.hip).
// Not shared: the stereo projection and Huber terms - the pose-only solver and the window smoother evaluate them in different
// association orders (fiz * s0 against fx * iz * inv_sigma), so merging them would change bits.
#pragma once
#include <hip/hip_runtime.h>

namespace sship {

__device__ __forceinline__ bool solver_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN and +-Inf
__device__ __forceinline__ bool solver_finitef(float v) { return fabsf(v) <= 3.4028234663852886e38f; }

// Tn = T Exp(delta), delta = (omega, v): R' = R (I + A W + B W^2), t' = t + R (I + B W + C W^2) v, W = [omega]x.  T row-major [R | t];
// no re-orthonormalisation.
__device__ __forceinline__ void se3_retract(const double* T, const double* delta, double* Tn) {
  const double wx = delta[0], wy = delta[1], wz = delta[2];
  const double th2 = wx * wx + wy * wy + wz * wz;
  double A, B, C;
  if (th2 < 1e-12) {
    A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; C = 1.0 / 6.0 - th2 / 120.0;
  } else {
    const double th = sqrt(th2), sh = sin(0.5 * th);
    const double st = sin(th);
    A = st / th; B = 2.0 * sh * sh / th2; C = (th - st) / (th2 * th);
  }
  const double W[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
  const double W2[3][3] = {{-(wy * wy + wz * wz), wx * wy, wx * wz}, {wx * wy, -(wx * wx + wz * wz), wy * wz}, {wx * wz, wy * wz, -(wx * wx + wy * wy)}};
  double E[3][3], u[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) E[i][j] = (i == j ? 1.0 : 0.0) + A * W[i][j] + B * W2[i][j];
    u[i] = delta[3 + i] + B * (W[i][0] * delta[3] + W[i][1] * delta[4] + W[i][2] * delta[5]) +
           C * (W2[i][0] * delta[3] + W2[i][1] * delta[4] + W2[i][2] * delta[5]);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) Tn[4 * i + j] = T[4 * i] * E[0][j] + T[4 * i + 1] * E[1][j] + T[4 * i + 2] * E[2][j];
    Tn[4 * i + 3] = T[4 * i + 3] + T[4 * i] * u[0] + T[4 * i + 1] * u[1] + T[4 * i + 2] * u[2];
  }
}

}  // namespace sship
