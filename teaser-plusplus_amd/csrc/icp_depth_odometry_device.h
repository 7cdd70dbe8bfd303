// icp_depth_odometry_device.h -- the per-pixel and per-pair rules of depth odometry that do not depend on the launch
// shape (include/teaser_hip.h, "Depth odometry"; kernels: kernels_depth_odometry.hip, host side: icp_depth_odometry.hip,
// design: DESIGN.md section 40): the records both sides read, the launchers, the image steps of one pixel, the 29 values
// a source pixel adds to the sums of an iteration, the 21 it adds to the information matrix, and what the one finishing
// thread of a pair does -- the solve, the pose update, the measures, the convergence test, the results.  The summation
// order (odo_sum_blocks), the solve (odo_solve) and the update (odo_update) are those of icp_odometry_device.h, by
// inclusion.  Nothing here uses a wave operation or LDS, so tests/depth_odometry_host_driver.cpp runs this very source
// in serial loops.
//
// The library is compiled with -ffp-contract=off: no product-add is fused, and every sum is written out left to right.
#pragma once

#include "icp_odometry_device.h"

namespace thip {

constexpr int kDodoPlanes = 11;
enum { kDodoDs, kDodoDt, kDodoVs, kDodoVt = 5, kDodoNt = 8 };  // the first plane of each image
enum { kDodoSumIter, kDodoSumInfo };                           // what a sums / finishing launch computes

// One pair (host-built, read-only on the device).
struct DodoDesc {
  int32_t width, height, levels, depth_format;
  int32_t blk_off[kOdoMaxLevels];  // the pair's first block among the blocks of level l
  int64_t img_off;      // first float of the pair's pyramid in the image pool (the layout of the contract)
  int64_t part_off;     // first of its ceil(n_0 / kOdoBlock) block partials (kOdoSums doubles each)
  int64_t trace_off;    // first trace record, -1: not asked for
  int64_t in_off[2];    // bytes: source depth, target depth, rows packed
  double fx, fy, cx, cy;
  double trunc, delta, depth_min, depth_max, rel_rmse, rel_fitness;
  float depth_scale;    // (float)depth_scale
  float thr;            // (float)(2.0 * depth_outlier_trunc)
};

// Mutable per-pair state.
struct DodoState {
  double T[16];          // the pose, row-major
  double fitness, rmse;  // the measures of the last executed iteration
  int32_t failed;        // 1: every later launch returns at once
  int32_t converged;     // 1: the level's remaining launches return at once; cleared behind the level's last iteration
  int32_t count;         // correspondences of the last executed iteration
  int32_t iterations;    // iterations executed
  int32_t converged_levels;  // bit l: level l converged
  int32_t pad;
};

struct DodoArgs {
  const DodoDesc* desc;
  DodoState* state;
  const int32_t* blk_pair;  // the pair of every block: the blocks of level 0 of all pairs, then level 1, ...
  const unsigned char* in;
  float* img;
  double* part;
  teaser_icp_depth_odometry_result_c* results;
  teaser_icp_depth_odometry_trace_c* trace;
  int batch, levels;
  int level_blk0[kOdoMaxLevels];  // first block of level l in blk_pair
  int level_nblk[kOdoMaxLevels];
};

// Steps 1 .. 4 of the contract.
void launch_dodo_preprocess(hipStream_t s, const DodoArgs& a);
// One iteration at `level`, record `iter` of the traces; first / last: of the level's iterations.
void launch_dodo_iteration(hipStream_t s, const DodoArgs& a, int level, int iter, int first, int last);
// Step 6 and the result records.
void launch_dodo_information(hipStream_t s, const DodoArgs& a);

__host__ __device__ __forceinline__ int dodo_w(const DodoDesc& d, int l) { return d.width >> l; }
__host__ __device__ __forceinline__ int dodo_h(const DodoDesc& d, int l) { return d.height >> l; }
__host__ __device__ __forceinline__ int64_t dodo_n(const DodoDesc& d, int l) { return (int64_t)dodo_w(d, l) * dodo_h(d, l); }
__host__ __device__ __forceinline__ int64_t dodo_blocks(const DodoDesc& d, int l) {
  return (dodo_n(d, l) + kOdoBlock - 1) / kOdoBlock;
}
// plane p of level l of the pair
__host__ __device__ __forceinline__ float* dodo_plane(float* img, const DodoDesc& d, int l, int p) {
  return img + d.img_off + kDodoPlanes * odo_pyramid_pixels(d.width, d.height, l) + p * dodo_n(d, l);
}

// Step 1 for pixel (y, x) of image `which` (0 source, 1 target).
__host__ __device__ __forceinline__ void dodo_px_convert(const DodoDesc& d, const unsigned char* in, float* img, int which,
                                                         int y, int x) {
  const unsigned char* row = in + d.in_off[which] + (int64_t)y * d.width * (d.depth_format == 0 ? 2 : 4);
  float zf;
  if (d.depth_format == 0) {
    uint16_t v;
    __builtin_memcpy(&v, row + 2 * (int64_t)x, 2);
    zf = (float)v / d.depth_scale;
  } else {
    zf = rgbd_load_f32(row + 4 * (int64_t)x);
  }
  if (!(__builtin_fabsf(zf) <= 3.4028234663852886e38f) || (double)zf <= d.depth_min || (double)zf > d.depth_max)
    zf = __builtin_nanf("");
  dodo_plane(img, d, 0, which)[(int64_t)y * d.width + x] = zf;
}

// Step 2 for pixel (y, x) of level l + 1 of image `which`.
__host__ __device__ __forceinline__ void dodo_px_down(const DodoDesc& d, float* img, int l, int which, int y, int x) {
  const int w = dodo_w(d, l), h = dodo_h(d, l);
  const float* D = dodo_plane(img, d, l, which);
  const float c = D[(int64_t)(2 * y) * w + 2 * x];
  float out = __builtin_nanf("");
  if (c == c) {
    const float k[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float s = 0.0f, ws = 0.0f;
    for (int dy = -2; dy <= 2; ++dy)
      for (int dx = -2; dx <= 2; ++dx) {
        const int yy = 2 * y + dy, xx = 2 * x + dx;
        if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
        const float v = D[(int64_t)yy * w + xx];
        if (v != v || !(__builtin_fabsf(v - c) < d.thr)) continue;
        const float wgt = k[dy + 2] * k[dx + 2];
        s = s + wgt * v;
        ws = ws + wgt;
      }
    out = odo_canon(s / ws);
  }
  dodo_plane(img, d, l + 1, which)[(int64_t)y * dodo_w(d, l + 1) + x] = out;
}

// Step 3 for pixel (y, x) of level l of image `which`.
__host__ __device__ __forceinline__ void dodo_px_vertex(const DodoDesc& d, float* img, int l, int which, int y, int x) {
  const int64_t at = (int64_t)y * dodo_w(d, l) + x;
  const float z = dodo_plane(img, d, l, which)[at];
  const int p0 = which == 0 ? kDodoVs : kDodoVt;
  float X = __builtin_nanf(""), Y = X, Z = X;
  if (z == z) {
    const double fx = odo_halved(d.fx, l), fy = odo_halved(d.fy, l), cx = odo_halved(d.cx, l), cy = odo_halved(d.cy, l);
    X = odo_canon((float)((((double)x - cx) * (double)z) * (1.0 / fx)));
    Y = odo_canon((float)((((double)y - cy) * (double)z) * (1.0 / fy)));
    Z = z;
  }
  dodo_plane(img, d, l, p0)[at] = X;
  dodo_plane(img, d, l, p0 + 1)[at] = Y;
  dodo_plane(img, d, l, p0 + 2)[at] = Z;
}

// Step 4 for pixel (y, x) of level l.
__host__ __device__ __forceinline__ void dodo_px_normal(const DodoDesc& d, float* img, int l, int y, int x) {
  const int w = dodo_w(d, l), h = dodo_h(d, l);
  const int64_t at = (int64_t)y * w + x;
  float N[3] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
  if (x + 1 < w && y + 1 < h) {
    float a[3], b[3];
    bool ok = true;
    for (int c = 0; c < 3; ++c) {
      const float* V = dodo_plane(img, d, l, kDodoVt + c);
      const float v0 = V[at], v1 = V[at + 1], v2 = V[at + w];
      ok = ok && v0 == v0 && v1 == v1 && v2 == v2;
      a[c] = v1 - v0;
      b[c] = v2 - v0;
    }
    if (ok) {
      const double a0 = a[0], a1 = a[1], a2 = a[2], b0 = b[0], b1 = b[1], b2 = b[2];
      const double m0 = b1 * a2 - b2 * a1, m1 = b2 * a0 - b0 * a2, m2 = b0 * a1 - b1 * a0;
      const double len = __builtin_sqrt((m0 * m0 + m1 * m1) + m2 * m2);
      if (len != 0.0 && rgbd_finite(len)) {
        N[0] = odo_canon((float)(m0 / len));
        N[1] = odo_canon((float)(m1 / len));
        N[2] = odo_canon((float)(m2 / len));
      }
    }
  }
  for (int c = 0; c < 3; ++c) dodo_plane(img, d, l, kDodoNt + c)[at] = N[c];
}

// The projection of steps 5 and 6 for source pixel s of level l at pose T: false when the pixel is skipped, else the
// transformed vertex p and the target pixel.
__host__ __device__ __forceinline__ bool dodo_px_project(const DodoDesc& d, const double* T, float* img, int l, int64_t s,
                                                         double* p, int64_t* tp) {
  const int w = dodo_w(d, l), h = dodo_h(d, l);
  const int64_t n = dodo_n(d, l);
  const float* V = dodo_plane(img, d, l, kDodoVs);
  const float P0f = V[s], P1f = V[n + s], P2f = V[2 * n + s];
  if (P0f != P0f || P1f != P1f || P2f != P2f) return false;
  const double P0 = P0f, P1 = P1f, P2 = P2f;
  p[0] = ((T[0] * P0 + T[1] * P1) + T[2] * P2) + T[3];
  p[1] = ((T[4] * P0 + T[5] * P1) + T[6] * P2) + T[7];
  p[2] = ((T[8] * P0 + T[9] * P1) + T[10] * P2) + T[11];
  if (!(p[2] > 0.0)) return false;
  const double fx = odo_halved(d.fx, l), fy = odo_halved(d.fy, l), cx = odo_halved(d.cx, l), cy = odo_halved(d.cy, l);
  const double x = ((fx * p[0]) / p[2] + cx) + 0.5, y = ((fy * p[1]) / p[2] + cy) + 0.5;
  if (!(x >= 0.0 && x < 2147483648.0) || !(y >= 0.0 && y < 2147483648.0)) return false;
  const int ut = (int)x, vt = (int)y;
  if (ut >= w || vt >= h) return false;
  *tp = (int64_t)vt * w + ut;
  return true;
}

// The kOdoSums values source pixel s of level l adds to the sums of `mode`; zeros for a pixel that is skipped.
__host__ __device__ __forceinline__ void dodo_px_values(int mode, const DodoDesc& d, const DodoState& st, float* img, int l,
                                                        int64_t s, bool in_level, double* v) {
  for (int k = 0; k < kOdoSums; ++k) v[k] = 0.0;
  if (!in_level) return;
  double p[3];
  int64_t tp;
  if (!dodo_px_project(d, st.T, img, l, s, p, &tp)) return;
  const int64_t n = dodo_n(d, l);
  const float* Vt = dodo_plane(img, d, l, kDodoVt);
  const float Q0f = Vt[tp], Q1f = Vt[n + tp], Q2f = Vt[2 * n + tp];
  if (Q0f != Q0f || Q1f != Q1f || Q2f != Q2f) return;
  const double e0 = p[0] - (double)Q0f, e1 = p[1] - (double)Q1f, e2 = p[2] - (double)Q2f;
  if (mode == kDodoSumInfo) {
    if (!(((e0 * e0 + e1 * e1) + e2 * e2) <= d.trunc * d.trunc)) return;
    const double x = Q0f, y = Q1f, z = Q2f;
    const double G[3][6] = {{0.0, z, -y, 1.0, 0.0, 0.0}, {-z, 0.0, x, 0.0, 1.0, 0.0}, {y, -x, 0.0, 0.0, 0.0, 1.0}};
    int k = 0;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) v[k++] = (G[0][i] * G[0][j] + G[1][i] * G[1][j]) + G[2][i] * G[2][j];
    v[kOdoSums - 1] = 1.0;
    return;
  }
  const float* Nt = dodo_plane(img, d, l, kDodoNt);
  const float N0f = Nt[tp], N1f = Nt[n + tp], N2f = Nt[2 * n + tp];
  if (N0f != N0f || N1f != N1f || N2f != N2f) return;
  const double N0 = N0f, N1 = N1f, N2 = N2f;
  const double r = (e0 * N0 + e1 * N1) + e2 * N2;
  const double ar = __builtin_fabs(r);
  if (!(ar <= d.trunc)) return;
  const double J[6] = {(-p[2]) * N1 + p[1] * N2, p[2] * N0 - p[0] * N2, (-p[1]) * N0 + p[0] * N1, N0, N1, N2};
  double dh, lh;
  if (ar < d.delta) {
    dh = r;
    lh = (0.5 * r) * r;
  } else {
    dh = r < 0.0 ? -d.delta : d.delta;
    lh = d.delta * (ar - 0.5 * d.delta);
  }
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) v[k++] = J[i] * J[j];
  for (int i = 0; i < 6; ++i) v[21 + i] = J[i] * dh;
  v[27] = lh;
  v[28] = 1.0;
}

// What the one finishing thread of a pair does with the totals tot[kOdoSums] of a sums launch.  kDodoSumIter: the solve,
// the update or the failure, the measures and the convergence test, record `rec` of the trace (NULL: none); first: the
// level's first iteration.  kDodoSumInfo: the result record.
__host__ __device__ inline void dodo_finish(int mode, const DodoDesc& d, DodoState& st, const double* tot, int level,
                                            int first, teaser_icp_depth_odometry_result_c* res,
                                            teaser_icp_depth_odometry_trace_c* rec) {
  if (mode == kDodoSumIter) {
    double x[6];
    st.count = (int32_t)tot[kOdoSums - 1];
    st.iterations += 1;
    const bool ok = odo_solve(tot, x);
    int conv = 0;
    if (ok) {
      odo_update(st.T, x);
      const double fitness = (double)st.count / (double)dodo_n(d, level);
      const double rmse = __builtin_sqrt(tot[27] / (double)st.count);
      if (!first && __builtin_fabs(fitness - st.fitness) <= d.rel_fitness * fitness &&
          __builtin_fabs(rmse - st.rmse) <= d.rel_rmse * rmse)
        conv = 1;
      st.fitness = fitness;
      st.rmse = rmse;
      if (conv) {
        st.converged = 1;
        st.converged_levels |= 1 << level;
      }
    } else {
      st.failed = 1;
      odo_identity(st.T);
    }
    if (rec) {
      rec->level = level, rec->executed = 1, rec->count = st.count, rec->failed = ok ? 0 : 1;
      rec->converged = conv, rec->reserved = 0;
      rec->e = rgbd_canonical(tot[27]);
      for (int k = 0; k < 21; ++k) rec->A[k] = rgbd_canonical(tot[k]);
      for (int k = 0; k < 6; ++k) rec->g[k] = rgbd_canonical(tot[21 + k]);
      for (int k = 0; k < 16; ++k) rec->pose[k] = st.T[k];
      rec->reserved2 = 0.0;
    }
    return;
  }
  res->success = st.failed ? 0 : 1;
  res->count = st.count;
  res->iterations = st.iterations;
  res->converged_levels = st.converged_levels;
  res->fitness = st.failed ? 0.0 : rgbd_canonical(st.fitness);
  res->inlier_rmse = st.failed ? 0.0 : rgbd_canonical(st.rmse);
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

}  // namespace thip
