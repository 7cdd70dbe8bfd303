// icp_fpfh_device.h -- the device code of the Open3D-form FPFH that does not depend on the launch shape
// (include/teaser_hip.h, "FPFH (Open3D form)"; kernels: kernels_fpfh.hip, host side: icp_fpfh.hip, design: DESIGN.md
// section 29): the pair features, the three bin indices, the SPFH row of a point and the steps of the FPFH recurrence.
// Nothing here uses a wave operation or LDS, so tests/fpfh_o3d_host_driver.cpp runs this very source in serial loops.
//
// Every dot product and squared length is (x x + y y) + z z, every component of a cross product a b - c d with both
// products rounded; the library is compiled with -ffp-contract=off, so no product-add is fused.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdet_math.h"

namespace thip {

constexpr int kFpfhBins = 11;             // per feature
constexpr int kFpfhDim = 3 * kFpfhBins;   // doubles of an SPFH / FPFH row
constexpr int kFpfhWaves = 4;             // FPFH pass: waves of a block; a block serves the 64 points of a map block

__host__ __device__ __forceinline__ double fpfh_dot(const double* a, const double* b) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

__host__ __device__ __forceinline__ void fpfh_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// The pair features f0, f1, f2 of (p1, n1) and (p2, n2) as the contract states them; a degenerate pair gives zeros.
__host__ __device__ __forceinline__ void fpfh_pair_features(const double* p1, const double* n1_in, const double* p2,
                                                            const double* n2_in, double* f) {
  f[0] = f[1] = f[2] = 0.0;
  double dp[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  const double f3 = __builtin_sqrt(fpfh_dot(dp, dp));
  if (f3 == 0.0) return;
  double n1[3] = {n1_in[0], n1_in[1], n1_in[2]}, n2[3] = {n2_in[0], n2_in[1], n2_in[2]};
  const double a1 = fpfh_dot(n1, dp) / f3, a2 = fpfh_dot(n2, dp) / f3;
  double f2 = a1;
  if (__builtin_fabs(a1) < __builtin_fabs(a2)) {
    for (int c = 0; c < 3; ++c) {
      const double t = n1[c];
      n1[c] = n2[c];
      n2[c] = t;
      dp[c] = -dp[c];
    }
    f2 = -a2;
  }
  double v[3], w[3];
  fpfh_cross(dp, n1, v);
  const double vn = __builtin_sqrt(fpfh_dot(v, v));
  if (vn == 0.0) return;
  for (int c = 0; c < 3; ++c) v[c] = v[c] / vn;
  fpfh_cross(n1, v, w);
  f[1] = fpfh_dot(v, n2);
  f[2] = f2;
  f[0] = fdet_atan2_d(fpfh_dot(w, n2), fpfh_dot(n1, n2));
}

// floor(x) clamped to a bin; a NaN (normals so large that a product overflowed) goes to bin 0.
__host__ __device__ __forceinline__ int fpfh_clamp_bin(double x) {
  const double h = __builtin_floor(x);
  return !(h >= 0.0) ? 0 : (h > 10.0 ? 10 : (int)h);
}

// The three bins of a pair: h[0] in [0, 10], h[1] in [11, 21], h[2] in [22, 32].
__host__ __device__ __forceinline__ void fpfh_bins(const double* f, int* h) {
  const double pi = 3.14159265358979323846;
  h[0] = fpfh_clamp_bin(11.0 * (f[0] + pi) / (2.0 * pi));
  h[1] = kFpfhBins + fpfh_clamp_bin(11.0 * (f[1] + 1.0) * 0.5);
  h[2] = 2 * kFpfhBins + fpfh_clamp_bin(11.0 * (f[2] + 1.0) * 0.5);
}

// m: the valid entries at the front of a list row of k slots (the rest hold index -1).
__host__ __device__ __forceinline__ int fpfh_list_length(const int32_t* idx, int k) {
  int m = 0;
  while (m < k && idx[m] >= 0) ++m;
  return m;
}

// The SPFH row of point i of a cloud (points / normals: the cloud's own arrays; idx: the m valid entries of its list)
// into hist[stride * bin], which the caller has cleared.  Position 0 of the list is skipped whatever it holds.
__host__ __device__ __forceinline__ void fpfh_spfh_row(const double* points, const double* normals, int64_t i,
                                                       const int32_t* idx, int m, double* hist, int stride) {
  if (m <= 1) return;
  const double c = 100.0 / (double)(m - 1);
  for (int k = 1; k < m; ++k) {
    const int64_t j = idx[k];
    double f[3];
    int h[3];
    fpfh_pair_features(points + 3 * i, normals + 3 * i, points + 3 * j, normals + 3 * j, f);
    fpfh_bins(f, h);
    for (int t = 0; t < 3; ++t) hist[stride * h[t]] += c;
  }
}

// The steps of the FPFH recurrence.  A neighbour's term: its SPFH entry over the SQUARED distance.
__host__ __device__ __forceinline__ double fpfh_term(double spfh, double d2) { return spfh / d2; }
// A group's sum becomes its scale.
__host__ __device__ __forceinline__ double fpfh_scale(double s) { return s != 0.0 ? 100.0 / s : s; }
// The end of a bin: two roundings.
__host__ __device__ __forceinline__ double fpfh_finish(double f, double scale, double own) {
  f = f * scale;
  return f + own;
}

// The FPFH row of a point, serially: spfh holds the rows of its cloud, idx / d2 the m valid entries of its list, own its
// own SPFH row.  (The kernel gives a lane to every bin and runs the same steps in the same order.)
__host__ __device__ __forceinline__ void fpfh_row(const double* spfh, const double* own, const int32_t* idx,
                                                  const double* d2, int m, double* out) {
  double S[3] = {0.0, 0.0, 0.0};
  for (int j = 0; j < kFpfhDim; ++j) out[j] = 0.0;
  if (m <= 1) return;
  for (int k = 1; k < m; ++k) {
    if (d2[k] == 0.0) continue;
    const double* row = spfh + (int64_t)kFpfhDim * idx[k];
    for (int j = 0; j < kFpfhDim; ++j) {
      const double val = fpfh_term(row[j], d2[k]);
      S[j / kFpfhBins] += val;
      out[j] += val;
    }
  }
  for (int g = 0; g < 3; ++g) S[g] = fpfh_scale(S[g]);
  for (int j = 0; j < kFpfhDim; ++j) out[j] = fpfh_finish(out[j], S[j / kFpfhBins], own[j]);
}

}  // namespace thip
