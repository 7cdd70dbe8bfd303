// icp_odometry_device.h -- the per-pixel and per-pair rules of RGB-D odometry that do not depend on the launch shape
// (include/teaser_hip.h, "RGB-D odometry"; kernels: kernels_odometry.hip, host side: icp_odometry.hip, design: DESIGN.md
// section 33): the records both sides read, the launchers, the image steps of one pixel, the correspondence of a source
// pixel, the values a target pixel adds to the sums, the order in which block sums are added, and what the one finishing
// thread of a pair does -- the solve, the pose update, the results.  Nothing here uses a wave operation or LDS, so
// tests/odometry_host_driver.cpp runs this very source in serial loops.
//
// The library is compiled with -ffp-contract=off: no product-add is fused, and every sum is written out left to right.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fdet_math.h"
#include "icp_rgbd_device.h"
#include "teaser_hip.h"

namespace thip {

constexpr int kOdoBlock = TEASER_HIP_ODOMETRY_BLOCK;  // target pixels per block of the stated summation order
constexpr int kOdoGroup = TEASER_HIP_ODOMETRY_GROUP;  // blocks per group of the stated summation order
constexpr int kOdoMaxLevels = TEASER_HIP_ODOMETRY_MAX_LEVELS;
constexpr int kOdoPlanes = 11;
constexpr int kOdoSums = 29;  // A by rows (21), g (6), e, the count
constexpr uint64_t kOdoEmptyKey = ~0ull;
enum { kOdoIs, kOdoIt, kOdoDs, kOdoDt, kOdoX, kOdoY, kOdoZ, kOdoItDx, kOdoItDy, kOdoDtDx, kOdoDtDy };
enum { kOdoSumNorm, kOdoSumIter, kOdoSumInfo };       // what a sums / finishing launch computes
enum { kOdoGaussIn, kOdoGaussLevel, kOdoSobel };      // what a filter launch computes

// One pair (host-built, read-only on the device).
struct OdoDesc {
  int32_t width, height, levels;
  int32_t depth_format, color_format, jacobian;
  int32_t blk_off[kOdoMaxLevels];  // the pair's first block among the blocks of level l
  int64_t img_off;      // first float of the pair's pyramid in the image pool (the layout of the contract)
  int64_t tmp_off;      // first float of its four scratch planes of n_0 pixels
  int64_t key_off;      // first of its n_0 keys
  int64_t part_off;     // first of its ceil(n_0 / kOdoBlock) block partials (kOdoSums doubles each)
  int64_t trace_off;    // first trace record, -1: not asked for
  int64_t in_off[4];    // bytes: source depth, source colour, target depth, target colour, rows packed
  double fx, fy, cx, cy;
  double depth_trunc, depth_diff_max, depth_min, depth_max;
  float depth_scale;    // (float)depth_scale
  float pad;
};

// Mutable per-pair state.
struct OdoState {
  double T[16];         // the pose, row-major
  double M[9], Kt[3];   // K R K^-1 and K t of T at the level of the next correspondence launch
  double scale_s, scale_t;
  int32_t failed;       // 1: every later launch returns at once
  int32_t count;        // correspondences of the last sums
  int32_t iterations;   // iterations executed
  int32_t normalise;    // 1: step 4 found correspondences, the intensities are scaled
};

struct OdoArgs {
  const OdoDesc* desc;
  OdoState* state;
  const int32_t* blk_pair;  // the pair of every block: the blocks of level 0 of all pairs, then level 1, ...
  const unsigned char* in;
  float* img;
  float* tmp;
  uint64_t* keys;
  double* part;
  teaser_icp_odometry_result_c* results;
  teaser_icp_odometry_trace_c* trace;
  int batch;
  int level_blk0[kOdoMaxLevels];  // first block of level l in blk_pair
  int level_nblk[kOdoMaxLevels];
};

// Steps 1 .. 7 of the contract for `levels` levels; the pose quantities are left for `next_level`.
void launch_odo_preprocess(hipStream_t s, const OdoArgs& a, int levels, int next_level);
// One iteration at `level`; record `iter` of the traces.
void launch_odo_iteration(hipStream_t s, const OdoArgs& a, int level, int next_level, int iter);
// The correspondences at the final pose, the information matrices and the result records.
void launch_odo_information(hipStream_t s, const OdoArgs& a);

__host__ __device__ __forceinline__ int odo_w(const OdoDesc& d, int l) { return d.width >> l; }
__host__ __device__ __forceinline__ int odo_h(const OdoDesc& d, int l) { return d.height >> l; }
__host__ __device__ __forceinline__ int64_t odo_n(const OdoDesc& d, int l) { return (int64_t)odo_w(d, l) * odo_h(d, l); }
__host__ __device__ __forceinline__ int64_t odo_pyramid_pixels(int width, int height, int levels) {
  int64_t n = 0;
  for (int l = 0; l < levels; ++l) n += (int64_t)(width >> l) * (height >> l);
  return n;
}
// plane p of level l of the pair
__host__ __device__ __forceinline__ float* odo_plane(float* img, const OdoDesc& d, int l, int p) {
  return img + d.img_off + kOdoPlanes * odo_pyramid_pixels(d.width, d.height, l) + p * odo_n(d, l);
}
__host__ __device__ __forceinline__ float* odo_tmp(float* tmp, const OdoDesc& d, int p) {
  return tmp + d.tmp_off + p * odo_n(d, 0);
}
__host__ __device__ __forceinline__ float odo_canon(float x) { return x != x ? __builtin_nanf("") : x; }
__host__ __device__ __forceinline__ double odo_halved(double x, int l) {
  for (int k = 0; k < l; ++k) x = x * 0.5;
  return x;
}

// Step 1 for pixel (y, x) of image `which` (0 source, 1 target): planes which (intensity) and 2 + which (depth) of the
// scratch.
__host__ __device__ __forceinline__ void odo_px_convert(const OdoDesc& d, const unsigned char* in, float* tmp, int which,
                                                        int y, int x) {
  const int64_t at = (int64_t)y * d.width + x;
  const unsigned char* drow = in + d.in_off[2 * which] + (int64_t)y * d.width * (d.depth_format == 0 ? 2 : 4);
  float zf;
  if (d.depth_format == 0) {
    uint16_t v;
    __builtin_memcpy(&v, drow + 2 * (int64_t)x, 2);
    zf = (float)v / d.depth_scale;
    if ((double)zf >= d.depth_trunc) zf = 0.0f;
  } else {
    zf = rgbd_load_f32(drow + 4 * (int64_t)x);
  }
  if (!(__builtin_fabsf(zf) <= 3.4028234663852886e38f) || (double)zf <= d.depth_min || (double)zf > d.depth_max)
    zf = __builtin_nanf("");
  odo_tmp(tmp, d, 2 + which)[at] = zf;
  const unsigned char* crow = in + d.in_off[2 * which + 1] + (int64_t)y * d.width * (d.color_format == 1 ? 3 : 4);
  float v;
  if (d.color_format == 1) {
    const unsigned char* px = crow + 3 * (int64_t)x;
    v = ((0.2990f * (float)px[0] + 0.5870f * (float)px[1]) + 0.1140f * (float)px[2]) / 255.0f;
  } else {
    v = rgbd_load_f32(crow + 4 * (int64_t)x);
  }
  odo_tmp(tmp, d, which)[at] = odo_canon(v);
}

// F(p; kh, kv)(y, x) of the contract over a w x h plane.
__host__ __device__ __forceinline__ float odo_filter3(const float* p, int w, int h, int y, int x, float kh0, float kh1,
                                                      float kh2, float kv0, float kv1, float kv2) {
  const int xm = x > 0 ? x - 1 : 0, xp = x < w - 1 ? x + 1 : w - 1;
  const int ym = y > 0 ? y - 1 : 0, yp = y < h - 1 ? y + 1 : h - 1;
  const float* r0 = p + (int64_t)ym * w;
  const float* r1 = p + (int64_t)y * w;
  const float* r2 = p + (int64_t)yp * w;
  const float H0 = (kh0 * r0[xm] + kh1 * r0[x]) + kh2 * r0[xp];
  const float H1 = (kh0 * r1[xm] + kh1 * r1[x]) + kh2 * r1[xp];
  const float H2 = (kh0 * r2[xm] + kh1 * r2[x]) + kh2 * r2[xp];
  return odo_canon((kv0 * H0 + kv1 * H1) + kv2 * H2);
}
__host__ __device__ __forceinline__ float odo_gauss(const float* p, int w, int h, int y, int x) {
  return odo_filter3(p, w, h, y, x, 0.25f, 0.5f, 0.25f, 0.25f, 0.5f, 0.25f);
}

// A filter step for pixel (y, x) of level l.  kOdoGaussIn: step 2.  kOdoGaussLevel: the Gaussian of planes 0 and 1 into
// scratch planes 0 and 1 (the first half of step 6).  kOdoSobel: step 7.
__host__ __device__ __forceinline__ void odo_px_filter(const OdoDesc& d, float* img, float* tmp, int l, int mode, int y,
                                                       int x) {
  const int w = odo_w(d, l), h = odo_h(d, l);
  const int64_t at = (int64_t)y * w + x;
  if (mode == kOdoGaussIn) {
    for (int p = 0; p < 4; ++p) odo_plane(img, d, 0, p)[at] = odo_gauss(odo_tmp(tmp, d, p), w, h, y, x);
  } else if (mode == kOdoGaussLevel) {
    for (int p = 0; p < 2; ++p) odo_tmp(tmp, d, p)[at] = odo_gauss(odo_plane(img, d, l, p), w, h, y, x);
  } else {
    const float* I = odo_plane(img, d, l, kOdoIt);
    const float* D = odo_plane(img, d, l, kOdoDt);
    odo_plane(img, d, l, kOdoItDx)[at] = odo_filter3(I, w, h, y, x, -1.0f, 0.0f, 1.0f, 1.0f, 2.0f, 1.0f);
    odo_plane(img, d, l, kOdoItDy)[at] = odo_filter3(I, w, h, y, x, 1.0f, 2.0f, 1.0f, -1.0f, 0.0f, 1.0f);
    odo_plane(img, d, l, kOdoDtDx)[at] = odo_filter3(D, w, h, y, x, -1.0f, 0.0f, 1.0f, 1.0f, 2.0f, 1.0f);
    odo_plane(img, d, l, kOdoDtDy)[at] = odo_filter3(D, w, h, y, x, 1.0f, 2.0f, 1.0f, -1.0f, 0.0f, 1.0f);
  }
}

__host__ __device__ __forceinline__ float odo_down(const float* p, int w, int y, int x) {
  const float* r0 = p + (int64_t)(2 * y) * w + 2 * x;
  const float* r1 = r0 + w;
  return odo_canon((((r0[0] + r0[1]) + r1[0]) + r1[1]) / 4.0f);
}

// The second half of step 6 for pixel (y, x) of level l + 1.
__host__ __device__ __forceinline__ void odo_px_down(const OdoDesc& d, float* img, const float* tmp, int l, int y, int x) {
  const int w = odo_w(d, l);
  const int64_t at = (int64_t)y * odo_w(d, l + 1) + x;
  for (int p = 0; p < 2; ++p) odo_plane(img, d, l + 1, p)[at] = odo_down(tmp + d.tmp_off + p * odo_n(d, 0), w, y, x);
  for (int p = 2; p < 7; ++p) odo_plane(img, d, l + 1, p)[at] = odo_down(odo_plane(img, d, l, p), w, y, x);
}

// Steps 4 (the scaling) and 5 for pixel (y, x) of level 0.
__host__ __device__ __forceinline__ void odo_px_scale_xyz(const OdoDesc& d, const OdoState& st, float* img, int y, int x) {
  const int64_t at = (int64_t)y * d.width + x;
  if (st.normalise) {
    float* Is = odo_plane(img, d, 0, kOdoIs);
    float* It = odo_plane(img, d, 0, kOdoIt);
    Is[at] = odo_canon((float)(st.scale_s * (double)Is[at]));
    It[at] = odo_canon((float)(st.scale_t * (double)It[at]));
  }
  const float z = odo_plane(img, d, 0, kOdoDs)[at];
  odo_plane(img, d, 0, kOdoX)[at] = odo_canon((float)((((double)x - d.cx) * (double)z) * (1.0 / d.fx)));
  odo_plane(img, d, 0, kOdoY)[at] = odo_canon((float)((((double)y - d.cy) * (double)z) * (1.0 / d.fy)));
  odo_plane(img, d, 0, kOdoZ)[at] = z;
}

// M and Kt of the state's pose at level l.
__host__ __device__ __forceinline__ void odo_level_pose(const OdoDesc& d, OdoState& st, int l) {
  const double f = odo_halved(d.fx, l), g = odo_halved(d.fy, l), a = odo_halved(d.cx, l), b = odo_halved(d.cy, l);
  const double* T = st.T;
  for (int r = 0; r < 3; ++r) {
    double A[3];
    for (int c = 0; c < 3; ++c)
      A[c] = r == 0 ? f * T[c] + a * T[8 + c] : (r == 1 ? g * T[4 + c] + b * T[8 + c] : T[8 + c]);
    st.M[3 * r] = A[0] / f;
    st.M[3 * r + 1] = A[1] / g;
    st.M[3 * r + 2] = (A[2] - (A[0] * a) / f) - (A[1] * b) / g;
  }
  st.Kt[0] = f * T[3] + a * T[11];
  st.Kt[1] = g * T[7] + b * T[11];
  st.Kt[2] = T[11];
}

// Source pixel s of level l: false when it is skipped, else its target pixel and its key (bits(zf) << 32) | s.
__host__ __device__ __forceinline__ bool odo_px_match(const OdoDesc& d, const OdoState& st, float* img, int l, int32_t s,
                                                      int32_t* pixel, uint64_t* key) {
  const int w = odo_w(d, l), h = odo_h(d, l);
  const float ds = odo_plane(img, d, l, kOdoDs)[s];
  if (ds != ds) return false;
  const int v = s / w, u = s - v * w;
  double q[3];
  for (int r = 0; r < 3; ++r)
    q[r] = (double)ds * ((st.M[3 * r] * (double)u + st.M[3 * r + 1] * (double)v) + st.M[3 * r + 2]) + st.Kt[r];
  if (!(q[2] > 0.0)) return false;
  const double x = q[0] / q[2] + 0.5, y = q[1] / q[2] + 0.5;
  if (!(__builtin_fabs(x) < 2147483648.0) || !(__builtin_fabs(y) < 2147483648.0)) return false;
  const int ut = (int)x, vt = (int)y;
  if (ut < 0 || ut >= w || vt < 0 || vt >= h) return false;
  const float dt = odo_plane(img, d, l, kOdoDt)[(int64_t)vt * w + ut];
  if (dt != dt) return false;
  if (!(__builtin_fabs(q[2] - (double)dt) <= d.depth_diff_max)) return false;
  const float zf = (float)q[2];
  if (!(zf <= 3.4028234663852886e38f)) return false;
  uint32_t bits;
  __builtin_memcpy(&bits, &zf, 4);
  *pixel = vt * w + ut;
  *key = ((uint64_t)bits << 32) | (uint32_t)s;
  return true;
}

// The kOdoSums values target pixel tp of level l adds to the sums of `mode`; zeros for an empty key.
__host__ __device__ __forceinline__ void odo_px_values(int mode, const OdoDesc& d, const OdoState& st, float* img, int l,
                                                       int32_t tp, uint64_t key, double* v) {
  for (int k = 0; k < kOdoSums; ++k) v[k] = 0.0;
  if (key == kOdoEmptyKey) return;
  const int32_t s = (int32_t)(uint32_t)key;
  const int w = odo_w(d, l);
  const int vt = tp / w, ut = tp - vt * w;
  v[kOdoSums - 1] = 1.0;
  if (mode == kOdoSumNorm) {
    v[0] = (double)odo_plane(img, d, l, kOdoIs)[s];
    v[1] = (double)odo_plane(img, d, l, kOdoIt)[tp];
    return;
  }
  if (mode == kOdoSumInfo) {
    const float zf = odo_plane(img, d, l, kOdoDt)[tp];
    const double x = (double)(float)((((double)ut - d.cx) * (double)zf) * (1.0 / d.fx));
    const double y = (double)(float)((((double)vt - d.cy) * (double)zf) * (1.0 / d.fy));
    const double z = (double)zf;
    const double G[3][6] = {{0.0, z, -y, 1.0, 0.0, 0.0}, {-z, 0.0, x, 0.0, 1.0, 0.0}, {y, -x, 0.0, 0.0, 0.0, 1.0}};
    int k = 0;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) v[k++] = (G[0][i] * G[0][j] + G[1][i] * G[1][j]) + G[2][i] * G[2][j];
    return;
  }
  const double f = odo_halved(d.fx, l), g = odo_halved(d.fy, l);
  const double* T = st.T;
  const double P0 = (double)odo_plane(img, d, l, kOdoX)[s], P1 = (double)odo_plane(img, d, l, kOdoY)[s];
  const double P2 = (double)odo_plane(img, d, l, kOdoZ)[s];
  const double p0 = ((T[0] * P0 + T[1] * P1) + T[2] * P2) + T[3];
  const double p1 = ((T[4] * P0 + T[5] * P1) + T[6] * P2) + T[7];
  const double p2 = ((T[8] * P0 + T[9] * P1) + T[10] * P2) + T[11];
  const double dp = (double)(odo_plane(img, d, l, kOdoIt)[tp] - odo_plane(img, d, l, kOdoIs)[s]);
  const double dg = (double)odo_plane(img, d, l, kOdoDt)[tp] - p2;
  const double iz = 1.0 / p2;
  const double gIx = 0.125 * (double)odo_plane(img, d, l, kOdoItDx)[tp];
  const double gIy = 0.125 * (double)odo_plane(img, d, l, kOdoItDy)[tp];
  double gDx = 0.125 * (double)odo_plane(img, d, l, kOdoDtDx)[tp];
  double gDy = 0.125 * (double)odo_plane(img, d, l, kOdoDtDy)[tp];
  if (gDx != gDx) gDx = 0.0;
  if (gDy != gDy) gDy = 0.0;
  const double c0 = (gIx * f) * iz, c1 = (gIy * g) * iz, c2 = (-(c0 * p0 + c1 * p1)) * iz;
  double J0[6] = {(-p2) * c1 + p1 * c2, p2 * c0 - p0 * c2, (-p1) * c0 + p0 * c1, c0, c1, c2};
  double r0 = dp;
  int k = 0;
  if (d.jacobian == 0) {
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) v[k++] = J0[i] * J0[j];
    for (int i = 0; i < 6; ++i) v[21 + i] = J0[i] * r0;
    v[27] = r0 * r0;
    return;
  }
  const double sI = __builtin_sqrt(1.0 - 0.968), sD = __builtin_sqrt(0.968);
  const double d0 = (gDx * f) * iz, d1 = (gDy * g) * iz, d2 = (-(d0 * p0 + d1 * p1)) * iz;
  for (int i = 0; i < 6; ++i) J0[i] = sI * J0[i];
  r0 = sI * r0;
  const double J1[6] = {sD * (((-p2) * d1 + p1 * d2) - p1), sD * ((p2 * d0 - p0 * d2) + p0), sD * ((-p1) * d0 + p0 * d1),
                        sD * d0, sD * d1, sD * (d2 - 1.0)};
  const double r1 = sD * dg;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) v[k++] = J0[i] * J0[j] + J1[i] * J1[j];
  for (int i = 0; i < 6; ++i) v[21 + i] = J0[i] * r0 + J1[i] * r1;
  v[27] = r0 * r0 + r1 * r1;
}

// Sum k of the nblk block partials at `part`, in the contract's order of groups.
__host__ __device__ __forceinline__ double odo_sum_blocks(const double* part, int64_t nblk, int k) {
  double total = 0.0;
  for (int64_t g0 = 0; g0 < nblk; g0 += kOdoGroup) {
    const int64_t g1 = g0 + kOdoGroup < nblk ? g0 + kOdoGroup : nblk;
    double gs = 0.0;
#pragma unroll 8
    for (int64_t b = g0; b < g1; ++b) gs += part[b * kOdoSums + k];
    total += gs;
  }
  return total;
}

__host__ __device__ __forceinline__ int64_t odo_blocks(const OdoDesc& d, int l) {
  return (odo_n(d, l) + kOdoBlock - 1) / kOdoBlock;
}

// A x = -g of the contract from tot = {A by rows, g}; false: the pair fails.
__host__ __device__ inline bool odo_solve(const double* tot, double* x) {
  double A[6][6], L[6][6], dd[6], y[6];
  int k = 0;
  for (int r = 0; r < 6; ++r)
    for (int q = r; q < 6; ++q) {
      A[r][q] = tot[k];
      A[q][r] = tot[k];
      ++k;
    }
  for (int j = 0; j < 6; ++j) {
    double sj = A[j][j];
    for (int m = 0; m < j; ++m) sj -= (L[j][m] * L[j][m]) * dd[m];
    if (!rgbd_finite(sj) || sj == 0.0) return false;
    dd[j] = sj;
    for (int i = j + 1; i < 6; ++i) {
      double t = A[i][j];
      for (int m = 0; m < j; ++m) t -= (L[i][m] * L[j][m]) * dd[m];
      L[i][j] = t / sj;
    }
  }
  const double det = ((((dd[0] * dd[1]) * dd[2]) * dd[3]) * dd[4]) * dd[5];
  if (!(__builtin_fabs(det) >= 1e-6)) return false;
  for (int i = 0; i < 6; ++i) {
    double t = -tot[21 + i];
    for (int m = 0; m < i; ++m) t -= L[i][m] * y[m];
    y[i] = t;
  }
  for (int i = 0; i < 6; ++i) y[i] = y[i] / dd[i];
  for (int i = 5; i >= 0; --i) {
    double t = y[i];
    for (int m = i + 1; m < 6; ++m) t -= L[m][i] * x[m];
    x[i] = t;
  }
  for (int i = 0; i < 6; ++i)
    if (!rgbd_finite(x[i])) return false;
  return true;
}

// T = U(x) T of the contract.
__host__ __device__ inline void odo_update(double* T, const double* x) {
  double sa, ca, sb, cb, sc, cc;
  fdet_sincos_d(x[0], &sa, &ca);
  fdet_sincos_d(x[1], &sb, &cb);
  fdet_sincos_d(x[2], &sc, &cc);
  const double U[12] = {cc * cb, (cc * sb) * sa - sc * ca, (cc * sb) * ca + sc * sa, x[3],
                        sc * cb, (sc * sb) * sa + cc * ca, (sc * sb) * ca - cc * sa, x[4],
                        -sb,     cb * sa,                  cb * ca,                  x[5]};
  double N[12];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) {
      const double v = (U[4 * r] * T[c] + U[4 * r + 1] * T[4 + c]) + U[4 * r + 2] * T[8 + c];
      N[4 * r + c] = c == 3 ? v + U[4 * r + 3] : v;
    }
  for (int k = 0; k < 12; ++k) T[k] = N[k];
}

__host__ __device__ __forceinline__ void odo_identity(double* T) {
  for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

// What the one finishing thread of a pair does with the totals tot[kOdoSums] of a sums launch.  kOdoSumNorm: the scales of
// step 4.  kOdoSumIter: the solve, the update or the failure, record `rec` of the trace (NULL: none).  kOdoSumInfo: the
// result record.  next_level >= 0: the pose quantities for the next correspondence launch.
__host__ __device__ inline void odo_finish(int mode, const OdoDesc& d, OdoState& st, const double* tot, int level,
                                           int next_level, teaser_icp_odometry_result_c* res,
                                           teaser_icp_odometry_trace_c* rec) {
  const double n = tot[kOdoSums - 1];
  if (mode == kOdoSumNorm) {
    st.normalise = n > 0.0 ? 1 : 0;
    st.scale_s = n > 0.0 ? 0.5 / (tot[0] / n) : 1.0;
    st.scale_t = n > 0.0 ? 0.5 / (tot[1] / n) : 1.0;
  } else if (mode == kOdoSumIter) {
    double x[6];
    st.count = (int32_t)n;
    st.iterations += 1;
    const bool ok = odo_solve(tot, x);
    if (ok) {
      odo_update(st.T, x);
    } else {
      st.failed = 1;
      odo_identity(st.T);
    }
    if (rec) {
      rec->level = level, rec->executed = 1, rec->count = st.count, rec->failed = ok ? 0 : 1;
      rec->e = rgbd_canonical(tot[27]);
      for (int k = 0; k < 21; ++k) rec->A[k] = rgbd_canonical(tot[k]);
      for (int k = 0; k < 6; ++k) rec->g[k] = rgbd_canonical(tot[21 + k]);
      for (int k = 0; k < 16; ++k) rec->pose[k] = st.T[k];
      rec->reserved[0] = rec->reserved[1] = 0.0;
    }
  } else {
    res->success = st.failed ? 0 : 1;
    if (!st.failed) st.count = (int32_t)n;
    res->count = st.count;
    res->iterations = st.iterations;
    res->reserved = 0;
    for (int k = 0; k < 16; ++k) res->transformation[k] = st.T[k];
    int k = 0;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) {
        const double v = st.failed ? 0.0 : rgbd_canonical(tot[k]);
        res->information[6 * i + j] = v;
        res->information[6 * j + i] = v;
        ++k;
      }
  }
  if (next_level >= 0) odo_level_pose(d, st, next_level);
}

}  // namespace thip
