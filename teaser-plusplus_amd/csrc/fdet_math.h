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

// The deterministic FP64 sine and cosine of the RGB-D odometry contract (include/teaser_hip.h, "RGB-D odometry"): + - x /
// and comparisons only, in the order written, for every finite x (a NaN or an infinity gives NaNs).
//   rounding:  rn(y) = (y + 6755399441055744.0) - 6755399441055744.0  (1.5 x 2^52: the nearest integer, halves to even,
//              for |y| < 2^51)
//   pi / 2 in three pieces P1 + P2 + P3 (P1 and P2 have 33 significant bits, so k P1 and k P2 are exact for |k| < 2^20)
//   large x:   if |x| >= 65536, for s = 0 .. 62 with c = 2^(1008 - 16 s):  if |x| >= 4 P1 c:  q = rn(x / (4 P1 c)),
//              x = ((x - q (4 P1 c)) - q (4 P2 c)) - q (4 P3 c).  This leaves |x| < 2 pi 65536.
//   quadrant:  k = rn(x 0.63661977236758138),  r = ((x - k P1) - k P2) - k P3,  z = r r
//   series:    S = 1, then for j = 10 .. 1: S = 1.0 - (z (1.0 / ((2j)(2j + 1)))) S;  sin r = r S
//              C = 1, then for j = 11 .. 1: C = 1.0 - (z (1.0 / ((2j - 1)(2j)))) C;  cos r = C
//   result:    n = k mod 4 (0 .. 3): (sin, cos) = (sin r, cos r), (cos r, -sin r), (-sin r, -cos r), (-cos r, sin r).
// Accuracy, measured against libm: at most 2 ulp and 2.3e-16 absolute for |x| < 65536.  A stage of
// the large-argument reduction rounds its remainder once, so beyond that the absolute error is about an ulp of the first
// remainder: 1.6e-11 up to 1e9, 1.9e-6 up to 1e15, and no correct digit from about 1e21 on (the results still lie on the
// unit circle).  The pose update's angles are far below 1.
__host__ __device__ inline double fdet_round_d(double y) { return (y + 6755399441055744.0) - 6755399441055744.0; }
__host__ __device__ inline void fdet_sincos_d(double x, double* s_out, double* c_out) {
  const double P1 = 1.57079632673412561417e+00, P2 = 6.07710050630396597660e-11, P3 = 2.02226624879595063154e-21;
  if (__builtin_fabs(x) >= 65536.0) {
    double c = 0x1p1008;
    for (int s = 0; s < 63; ++s) {
      const double m1 = (4.0 * P1) * c, m2 = (4.0 * P2) * c, m3 = (4.0 * P3) * c;
      if (__builtin_fabs(x) >= m1) {
        const double q = fdet_round_d(x / m1);
        x = ((x - q * m1) - q * m2) - q * m3;
      }
      c = c * 0x1p-16;
    }
  }
  const double k = fdet_round_d(x * 0.63661977236758138);
  const double r = ((x - k * P1) - k * P2) - k * P3;
  const double z = r * r;
  double S = 1.0, C = 1.0;
#pragma unroll  // (the quotients fold to constants: correctly rounded at compile time as at run time)
  for (int j = 10; j >= 1; --j) S = 1.0 - (z * (1.0 / (double)((2 * j) * (2 * j + 1)))) * S;
#pragma unroll
  for (int j = 11; j >= 1; --j) C = 1.0 - (z * (1.0 / (double)((2 * j - 1) * (2 * j)))) * C;
  const double sr = r * S, cr = C;
  // k is an integer below 2^19 in magnitude (two's complement gives k mod 4), or a NaN whose results are NaNs anyway
  const int n = k == k ? (int)(long long)k & 3 : 0;
  *s_out = n == 0 ? sr : (n == 1 ? cr : (n == 2 ? -sr : -cr));
  *c_out = n == 0 ? cr : (n == 1 ? -sr : (n == 2 ? -cr : sr));
}

}  // namespace thip
