// plane_device.h -- what the host side (plane.hip) and the kernels (kernels_plane.hip) of RANSAC plane segmentation
// share: the records both sides read, the launchers, and the arithmetic as one-lane functions.  The contract is written
// out in include/teaser_hip.h, "Plane segmentation"; the expression order here IS that contract (the build sets
// -ffp-contract=off).  The one-lane functions are also what tests/plane_host_driver.cpp runs on the CPU.
#pragma once

#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "ransac_device.h"  // rs_draw: the splitmix64 finaliser of the tuple-test and RANSAC contracts

namespace thip {

constexpr int PL_MAX_N = 8;     // ransac_n <= 8
constexpr int PL_BLOCK = 256;   // positions per block of the stated summation order, and lanes per workgroup
constexpr int PL_GROUP = 64;    // blocks per group of the stated summation order
constexpr int PL_TILE = 64;     // hypotheses per tile of the score kernel: one per lane of a wave
constexpr int PL_WAVES = PL_BLOCK / PL_TILE;  // waves of a score workgroup: each takes one block of points
constexpr int PL_FLAG_VALID = 1;

struct PlDesc {  // one problem
  int64_t pt_off;    // its first point in the packed cloud array (in points)
  int64_t blk_off;   // its first block in the finish partials (in blocks)
  int64_t grp_off;   // its first group in the finish partials (in groups)
  int64_t part_grp;  // its first group in the score partials of one point wave (in groups)
  uint64_t seed;
  double d;          // distance_threshold
  int32_t n, ransac_n;
  int32_t run, pad;  // run = 0: n < ransac_n, no trial is drawn
};

inline __host__ __device__ int64_t pl_blocks(int32_t n) { return ((int64_t)n + PL_BLOCK - 1) / PL_BLOCK; }
inline __host__ __device__ int64_t pl_groups(int32_t n) { return (pl_blocks(n) + PL_GROUP - 1) / PL_GROUP; }

// The per-trial arrays of one chunk, [problem][trial of the chunk].
struct PlSlot {
  double* E;         // the sum of the inlier distances, carried across the point waves
  int32_t* count;    // the inliers, likewise
  uint8_t* flags;    // bit 0: not degenerate
  double* model;     // 4 per trial, zero when degenerate
  int32_t* samples;  // PL_MAX_N per trial, or NULL (the stage call asks for them)
  const int32_t* n;  // [problem] trials of this chunk
};

// The partials of one point wave: W groups of every problem, problem b's from group slot part_grp.
struct PlPart {
  int32_t* bcnt;  // [(group slot) 64 + block of the group][trial of the chunk]
  double* bsum;
  int32_t* gcnt;  // [group slot][trial of the chunk]
  double* gsum;
};

// The finish: the mask under the winning plane and the two fixed-order reductions of the refit.
struct PlFin {
  const int64_t* best;  // [problem] the winning trial, -1: none
  uint8_t* mask;        // [point of the packed array]
  double* bsum;         // 6 per finish block
  int32_t* bcnt;        // per finish block
  double* gsum;         // 6 per finish group
  int32_t* gcnt;        // per finish group
  double* centroid;     // 3 per problem
  int32_t* m;           // [problem] the inliers
  double* win;          // 4 per problem: the winning trial's plane
  double* plane;        // 4 per problem: the refit
};

// the model kernel of one chunk: trials first .. first + n[b] - 1 of every problem
void launch_plane_models(hipStream_t s, int batch, int chunk, int max_n, const PlDesc* desc, const double* pts,
                         const PlSlot& slot, int64_t first);
// the score kernel and the two combine kernels over groups g0 .. g0 + W - 1 of every problem's points
void launch_plane_score(hipStream_t s, int batch, int chunk, int max_n, const PlDesc* desc, const double* pts,
                        const PlSlot& slot, const PlPart& part, int g0, int W);
// the finish kernels: winner, mask and 3 sums, groups, centroid, 6 sums, groups, determinant step
void launch_plane_finish(hipStream_t s, int batch, int max_points, const PlDesc* desc, const double* pts,
                         const PlFin& fin);

// abc / len and the offset through `anchor`; false and the zero plane when len is zero or not finite.
__host__ __device__ inline bool pl_normalise(double a, double b, double c, const double* anchor, double* plane) {
  const double len = sqrt((a * a + b * b) + c * c);
  if (!(len > 0.0) || !(len <= 1.7976931348623157e308)) {
    plane[0] = plane[1] = plane[2] = plane[3] = 0.0;
    return false;
  }
  a /= len;
  b /= len;
  c /= len;
  const double s = (a * anchor[0] + b * anchor[1]) + c * anchor[2];
  plane[0] = a;
  plane[1] = b;
  plane[2] = c;
  plane[3] = -s;
  return true;
}

// Steps 3 .. 6 of plane_from_points: S = {xx, xy, xz, yy, yz, zz} of the centred points.
__host__ __device__ inline bool pl_from_sums(const double* centroid, const double* S, double* plane) {
  const double xx = S[0], xy = S[1], xz = S[2], yy = S[3], yz = S[4], zz = S[5];
  const double det_x = yy * zz - yz * yz, det_y = xx * zz - xz * xz, det_z = xx * yy - xy * xy;
  int axis = 0;
  double det_max = det_x;
  if (det_y > det_max) {
    axis = 1;
    det_max = det_y;
  }
  if (det_z > det_max) axis = 2;
  double a, b, c;
  if (axis == 0) {
    a = det_x;
    b = xz * yz - xy * zz;
    c = xy * yz - xz * yy;
  } else if (axis == 1) {
    a = xz * yz - xy * zz;
    b = det_y;
    c = xy * xz - yz * xx;
  } else {
    a = xy * yz - xz * yy;
    b = xy * xz - yz * xx;
    c = det_z;
  }
  return pl_normalise(a, b, c, centroid, plane);
}

// One trial up to its model: the draws, then the cross product (ransac_n = 3) or plane_from_points over the samples
// in sample order.  P = the problem's points.  Returns the flag byte.
__host__ __device__ inline int pl_model(const PlDesc& D, const double* P, int64_t trial, int32_t* smp, double* plane) {
  const int n = D.ransac_n;
  for (int k = 0; k < PL_MAX_N; ++k)  // constant trip counts and a test: the arrays stay in registers
    smp[k] = k < n ? (int32_t)(rs_draw(D.seed, (uint64_t)n * (uint64_t)trial + (uint64_t)k + 1ull) % (uint64_t)D.n) : -1;
  if (n == 3) {
    const double* p0 = P + 3 * (int64_t)smp[0];
    const double* p1 = P + 3 * (int64_t)smp[1];
    const double* p2 = P + 3 * (int64_t)smp[2];
    const double ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
    const double vx = p2[0] - p0[0], vy = p2[1] - p0[1], vz = p2[2] - p0[2];
    const double a = uy * vz - uz * vy, b = uz * vx - ux * vz, c = ux * vy - uy * vx;
    return pl_normalise(a, b, c, p0, plane) ? PL_FLAG_VALID : 0;
  }
  double cen[3] = {0.0, 0.0, 0.0}, S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < PL_MAX_N; ++k) {
    if (k >= n) continue;
    const double* p = P + 3 * (int64_t)smp[k];
    cen[0] += p[0];
    cen[1] += p[1];
    cen[2] += p[2];
  }
  cen[0] /= (double)n;
  cen[1] /= (double)n;
  cen[2] /= (double)n;
  for (int k = 0; k < PL_MAX_N; ++k) {
    if (k >= n) continue;
    const double* p = P + 3 * (int64_t)smp[k];
    const double rx = p[0] - cen[0], ry = p[1] - cen[1], rz = p[2] - cen[2];
    S[0] += rx * rx;
    S[1] += rx * ry;
    S[2] += rx * rz;
    S[3] += ry * ry;
    S[4] += ry * rz;
    S[5] += rz * rz;
  }
  return pl_from_sums(cen, S, plane) ? PL_FLAG_VALID : 0;
}

__host__ __device__ inline double pl_dist(const double* w, const double* p) {
  return fabs(((w[0] * p[0] + w[1] * p[1]) + w[2] * p[2]) + w[3]);
}

// One block of the score: the m points at P in index order, from 0.
__host__ __device__ inline void pl_score_block(const double* w, double d, const double* P, int m, int32_t* count,
                                               double* sum) {
  int32_t c = 0;
  double bs = 0.0;
  for (int i = 0; i < m; ++i) {
    const double dist = pl_dist(w, P + 3 * i);
    if (dist < d) {
      ++c;
      bs += dist;
    }
  }
  *count = c;
  *sum = bs;
}

// One block of the finish's first pass: the mask under the winning plane and the coordinate sums of the inliers.
__host__ __device__ inline void pl_fin_block_mask(bool any, const double* w, double d, const double* P, int m,
                                                  uint8_t* mask, int32_t* count, double* S) {
  int32_t c = 0;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int i = 0; i < m; ++i) {
    const bool in = any && pl_dist(w, P + 3 * i) < d;
    mask[i] = in ? 1 : 0;
    if (in) {
      ++c;
      sx += P[3 * i];
      sy += P[3 * i + 1];
      sz += P[3 * i + 2];
    }
  }
  *count = c;
  S[0] = sx;
  S[1] = sy;
  S[2] = sz;
  S[3] = S[4] = S[5] = 0.0;
}

// ... and of its second pass: the six product sums of the centred inliers.
__host__ __device__ inline void pl_fin_block_cov(const double* cen, const double* P, int m, const uint8_t* mask,
                                                 double* S) {
  double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
  for (int i = 0; i < m; ++i) {
    if (!mask[i]) continue;
    const double rx = P[3 * i] - cen[0], ry = P[3 * i + 1] - cen[1], rz = P[3 * i + 2] - cen[2];
    xx += rx * rx;
    xy += rx * ry;
    xz += rx * rz;
    yy += ry * ry;
    yz += ry * rz;
    zz += rz * rz;
  }
  S[0] = xx;
  S[1] = xy;
  S[2] = xz;
  S[3] = yy;
  S[4] = yz;
  S[5] = zz;
}

__host__ __device__ inline double pl_rmse(int32_t count, double E) {
  return count > 0 ? E / sqrt((double)count) : 0.0;
}

}  // namespace thip
