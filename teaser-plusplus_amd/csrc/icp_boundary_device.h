// icp_boundary_device.h -- the per-point rule of boundary-point detection that does not depend on the launch shape
// (include/teaser_hip.h, "Boundary points"; kernel: kernels_boundary.hip, host side: icp_boundary.hip, design: DESIGN.md
// section 30): the tangent frame of a point, the angle of a neighbour in it, and the largest gap of a sorted array of
// angles.  Nothing here uses a wave operation or LDS, so tests/boundary_host_driver.cpp runs this very source in serial
// loops.
//
// Every dot product is (x x + y y) + z z, every component of a cross product a b - c d with both products rounded; the
// library is compiled with -ffp-contract=off, so no product-add is fused.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdet_math.h"
#include "icp_fpfh_device.h"

namespace thip {

constexpr int kBoundaryWaves = 4;     // waves of a block; a block serves the 64 points of a map block
constexpr int kBoundarySlots = 128;   // angle slots of a wave, two per lane: a list holds at most 99 neighbours

__host__ __device__ __forceinline__ bool boundary_finite(double x) { return __builtin_fabs(x) <= 1.7976931348623157e308; }

// Eigen's unitOrthogonal of the normal n (v) and u = cross(n, v).  false: a component of u or v is not finite.
__host__ __device__ __forceinline__ bool boundary_frame(const double* n, double* u, double* v) {
  const double ax = __builtin_fabs(n[0]), ay = __builtin_fabs(n[1]), az = __builtin_fabs(n[2]);
  if (!(ax <= 1e-12 * az) || !(ay <= 1e-12 * az)) {
    const double s = 1.0 / __builtin_sqrt(n[0] * n[0] + n[1] * n[1]);
    v[0] = -n[1] * s;
    v[1] = n[0] * s;
    v[2] = 0.0;
  } else {
    const double s = 1.0 / __builtin_sqrt(n[1] * n[1] + n[2] * n[2]);
    v[0] = 0.0;
    v[1] = -n[2] * s;
    v[2] = n[1] * s;
  }
  fpfh_cross(n, v, u);
  bool ok = true;
  for (int c = 0; c < 3; ++c) ok = ok && boundary_finite(u[c]) && boundary_finite(v[c]);
  return ok;
}

// The angle of the neighbour q of the point p in the frame (u, v); a coincident neighbour lies along u.
__host__ __device__ __forceinline__ double boundary_angle(const double* p, const double* q, const double* u,
                                                          const double* v) {
  const double d[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
  if (d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0) return 0.0;
  return fdet_atan2_d(fpfh_dot(v, d), fpfh_dot(u, d));
}

// One step of the gap rule.
__host__ __device__ __forceinline__ double boundary_step(double max_gap, double d) { return d > max_gap ? d : max_gap; }
// The wrap term of the first and the last sorted angle.
__host__ __device__ __forceinline__ double boundary_wrap(double first, double last) {
  const double pi = 3.14159265358979323846;
  return (2.0 * pi - last) + first;
}

// max_gap of count >= 1 angles in ascending order, none of them a NaN.
__host__ __device__ __forceinline__ double boundary_max_gap(const double* a, int count) {
  double g = 0.0;
  for (int t = 0; t + 1 < count; ++t) g = boundary_step(g, a[t + 1] - a[t]);
  return boundary_step(g, boundary_wrap(a[0], a[count - 1]));
}

__host__ __device__ __forceinline__ bool boundary_is_boundary(double max_gap, double threshold) {
  return max_gap > threshold;
}

}  // namespace thip
