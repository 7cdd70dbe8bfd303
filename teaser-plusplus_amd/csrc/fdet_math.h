// fdet_math.h -- the deterministic FP64 arc tangent both FPFH forms use (kernels_features.hip: the PCL form;
// icp_fpfh_device.h: the Open3D form): IEEE double basic operations only, in a fixed order, so the device, a host
// compiler without product-add fusion and a numpy restatement give the same bits.  libm's atan2 is not portable to the
// last bit.
#pragma once

#include <hip/hip_runtime.h>

namespace thip {

__host__ __device__ inline double fdet_atan_d(double x) {  // |x| <= 1: two argument halvings, then the Taylor series
  double t = x / (1.0 + __builtin_sqrt(1.0 + x * x));
  t = t / (1.0 + __builtin_sqrt(1.0 + t * t));
  const double t2 = t * t;
  double s = 0.0;
#pragma unroll  // (the quotients 1 / (2k + 1) fold to constants: correctly rounded at compile time as at run time)
  for (int k = 24; k >= 0; --k) s = 1.0 / (double)(2 * k + 1) - t2 * s;
  return 4.0 * (t * s);
}
__host__ __device__ inline double fdet_atan2_d(double y, double x) {
  const double pi = 3.14159265358979323846;
  if (x == 0.0 && y == 0.0) return 0.0;
  const double ax = __builtin_fabs(x), ay = __builtin_fabs(y);
  double a = (ax >= ay) ? fdet_atan_d(ay / ax) : pi / 2 - fdet_atan_d(ax / ay);
  if (x < 0.0) a = pi - a;
  return (y < 0.0) ? -a : a;
}

}  // namespace thip
