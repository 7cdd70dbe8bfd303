// svd3.h -- the device 3x3 SVD rotation shared by the estimators (kernels_estimate.hip) and ICP (kernels_icp.hip).
// One definition, included by both translation units, so both compile the same arithmetic (-ffp-contract=off);
// `inline` keeps the header valid under relocatable device code (-fgpu-rdc) too.
#pragma once

#include <math.h>

#include <hip/hip_runtime.h>

namespace thip {

// ------------------------------------------------------------------------------------------
// 3x3 SVD rotation (utils.h:121-136): R = V diag(1,1,det(U)det(V)) U^T, H = U S V^T.
// One-sided (Hestenes) Jacobi on the columns of H; row-major 3x3 arrays; run by one thread.
// ------------------------------------------------------------------------------------------
__device__ inline double det3(const double* M) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) +
         M[2] * (M[3] * M[7] - M[4] * M[6]);
}

__device__ inline void svd_rot3(const double* H, double* R) {
  double B[9], V[9];
  for (int i = 0; i < 9; ++i) {
    B[i] = H[i];
    V[i] = (i % 4 == 0) ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p) {
      for (int q = p + 1; q < 3; ++q) {
        double alpha = 0, beta = 0, gamma = 0;
        for (int r = 0; r < 3; ++r) {
          alpha += B[3 * r + p] * B[3 * r + p];
          beta += B[3 * r + q] * B[3 * r + q];
          gamma += B[3 * r + p] * B[3 * r + q];
        }
        // converged pair: the columns are orthogonal to working precision.  (The threshold used to be 1e-17, below
        // the rounding noise of gamma itself (~1e-16 sqrt(alpha beta)): most calls then ran all 60 sweeps -- ~50 us
        // of one thread's FP64 divisions and square roots per GNC iteration, the larger part of the rotation stage.)
        if (gamma == 0.0 || fabs(gamma) <= 1e-15 * sqrt(alpha * beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int r = 0; r < 3; ++r) {
          const double bp = B[3 * r + p], bq = B[3 * r + q];
          B[3 * r + p] = c * bp - s * bq;
          B[3 * r + q] = s * bp + c * bq;
          const double vp = V[3 * r + p], vq = V[3 * r + q];
          V[3 * r + p] = c * vp - s * vq;
          V[3 * r + q] = s * vp + c * vq;
        }
      }
    }
    if (!rotated) break;
  }
  double sig[3];
  for (int c = 0; c < 3; ++c)
    sig[c] = sqrt(B[c] * B[c] + B[3 + c] * B[3 + c] + B[6 + c] * B[6 + c]);
  // order columns by descending singular value
  int i0 = 0, i1 = 1, i2 = 2;
  if (sig[i1] > sig[i0]) { int t = i0; i0 = i1; i1 = t; }
  if (sig[i2] > sig[i0]) { int t = i0; i0 = i2; i2 = t; }
  if (sig[i2] > sig[i1]) { int t = i1; i1 = i2; i2 = t; }
  const double s0 = sig[i0], s1 = sig[i1], s2 = sig[i2];
  double u0[3], u1[3], u2[3], v0[3], v1[3], v2[3];
  for (int r = 0; r < 3; ++r) {
    v0[r] = V[3 * r + i0];
    v1[r] = V[3 * r + i1];
    v2[r] = V[3 * r + i2];
  }
  const double tiny = 1e-300;
  if (s0 > tiny) {
    for (int r = 0; r < 3; ++r) u0[r] = B[3 * r + i0] / s0;
  } else {
    u0[0] = 1; u0[1] = 0; u0[2] = 0;
  }
  if (s1 > tiny && s1 > 1e-15 * s0) {
    for (int r = 0; r < 3; ++r) u1[r] = B[3 * r + i1] / s1;
  } else {
    const int k = (fabs(u0[0]) <= fabs(u0[1]) && fabs(u0[0]) <= fabs(u0[2])) ? 0
                  : (fabs(u0[1]) <= fabs(u0[2]) ? 1 : 2);
    double nn = 0;
    for (int r = 0; r < 3; ++r) {
      u1[r] = (r == k ? 1.0 : 0.0) - u0[k] * u0[r];
      nn += u1[r] * u1[r];
    }
    nn = sqrt(nn);
    for (int r = 0; r < 3; ++r) u1[r] /= nn;
  }
  if (s2 > tiny && s2 > 1e-15 * s0) {
    for (int r = 0; r < 3; ++r) u2[r] = B[3 * r + i2] / s2;
  } else {
    u2[0] = u0[1] * u1[2] - u0[2] * u1[1];
    u2[1] = u0[2] * u1[0] - u0[0] * u1[2];
    u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
  }
  double U[9], Vs[9];
  for (int r = 0; r < 3; ++r) {
    U[3 * r] = u0[r]; U[3 * r + 1] = u1[r]; U[3 * r + 2] = u2[r];
    Vs[3 * r] = v0[r]; Vs[3 * r + 1] = v1[r]; Vs[3 * r + 2] = v2[r];
  }
  if (det3(U) * det3(Vs) < 0) {  // utils.h:131-133
    Vs[2] = -Vs[2]; Vs[5] = -Vs[5]; Vs[8] = -Vs[8];
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      R[3 * r + c] = Vs[3 * r] * U[3 * c] + Vs[3 * r + 1] * U[3 * c + 1] + Vs[3 * r + 2] * U[3 * c + 2];
}

}  // namespace thip
