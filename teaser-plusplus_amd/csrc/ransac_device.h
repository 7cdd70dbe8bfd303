// ransac_device.h -- what the host side (ransac.hip) and the kernels (kernels_ransac.hip) of RANSAC registration on
// correspondences share: the records both sides read, the launchers, and the arithmetic of one trial as one-lane
// functions.  The contract is written out in include/teaser_hip.h, "RANSAC registration on correspondences"; the
// expression order here IS that contract (the build sets -ffp-contract=off).  The one-lane functions are also what
// tests/ransac_host_driver.cpp runs on the CPU, one lane at a time.
#pragma once

#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "svd3.h"

namespace thip {

constexpr int RS_MAX_N = 8;        // ransac_n <= 8
constexpr int RS_BLOCK = 256;      // lanes per workgroup, and pairs per block of the stated summation order
constexpr int RS_LIST_CAP = 64;    // improvement records one (problem, chunk) hands over per prefix launch
constexpr int RS_FLAG_EDGE = 1, RS_FLAG_DIST = 2, RS_FLAG_SCORED = 4;

struct RsDesc {  // one problem
  int64_t pair_off;                    // its first 48-byte pair record
  int64_t src_off, dst_off, corr_off;  // its first point (in points) of either cloud and its first pair (in pairs)
  uint64_t seed;
  double r2, s, d;  // r r; the edge-length threshold (0: off); the distance threshold (0: off)
  int32_t ncorr, ransac_n;
  int32_t run, pad;  // run = 0: ncorr < ransac_n, no trial is drawn
};

struct RsBest {
  double rmse;
  int32_t count, pad;
};

struct RsEntry {  // one strict improvement: everything the host needs of the trial
  int64_t trial;
  double sum;
  double T[12];
  int32_t count, pad;
};

// The arrays of one chunk, [problem][lane of the chunk] unless noted.
struct RsSlot {
  double* T;         // 12 per trial: rows 0..2 of the 4 x 4
  uint8_t* flags;
  int32_t* count;
  double* sum;
  int32_t* surv;     // the lanes that passed their checkers, in any order
  int32_t* nsurv;    // [problem]
  int32_t* samples;  // RS_MAX_N per trial, or NULL (the stage call asks for them)
  const int32_t* n;  // [problem] trials of this chunk
  const RsBest* best_in;  // [problem] the best before this chunk
  RsBest* best_out;       // [problem] ... and after it
  int32_t* n_imp;         // [problem] strict improvements in this chunk
  RsEntry* entries;       // [problem][RS_LIST_CAP]
};

void launch_ransac_pack(hipStream_t s, int batch, int max_corr, const RsDesc* desc, const double* src,
                        const double* dst, const int32_t* corr, double* pairs);
// the hypothesis kernel and the score kernel of one chunk: trials first .. first + n[b] - 1 of every problem
void launch_ransac_chunk(hipStream_t s, int batch, int chunk, int max_n, const RsDesc* desc, const double* pairs,
                         const RsSlot& slot, int64_t first);
// the prefix kernel: the strict improvements number skip .. skip + RS_LIST_CAP - 1 of the chunk, and best_out
void launch_ransac_prefix(hipStream_t s, int batch, int chunk, const RsSlot& slot, int64_t first, int32_t skip);

// splitmix64's output for the state seed + n 0x9E3779B97F4A7C15 (the tuple test's draw)
__host__ __device__ inline uint64_t rs_draw(uint64_t seed, uint64_t n) {
  uint64_t z = seed + n * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ inline double rs_dist(const double* a, const double* b) {
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

// apply(T, p) and the squared distance to q; rec = {p, q}
__host__ __device__ inline double rs_pair_d2(const double* T, const double* rec) {
  const double x = ((T[0] * rec[0] + T[1] * rec[1]) + T[2] * rec[2]) + T[3];
  const double y = ((T[4] * rec[0] + T[5] * rec[1]) + T[6] * rec[2]) + T[7];
  const double z = ((T[8] * rec[0] + T[9] * rec[1]) + T[10] * rec[2]) + T[11];
  const double dx = x - rec[3], dy = y - rec[4], dz = z - rec[5];
  return (dx * dx + dy * dy) + dz * dz;
}

// One trial up to its score: the draws, the edge-length test, the estimate, the distance test.  pairs = the problem's
// records; smp receives the ransac_n draws; T the 12 entries (the identity when the edge-length test fails).
__device__ inline int rs_hypothesis(const RsDesc& D, const double* pairs, int64_t trial, int32_t* smp, double* T) {
  const int n = D.ransac_n;
  for (int k = 0; k < n; ++k)
    smp[k] = (int32_t)(rs_draw(D.seed, (uint64_t)n * (uint64_t)trial + (uint64_t)k + 1ull) % (uint64_t)D.ncorr);
  for (int k = 0; k < 12; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
  if (D.s > 0.0)
    for (int a = 0; a < n; ++a)
      for (int b = a + 1; b < n; ++b) {
        const double* ra = pairs + 6 * (int64_t)smp[a];
        const double* rb = pairs + 6 * (int64_t)smp[b];
        const double ls = rs_dist(ra, rb), lt = rs_dist(ra + 3, rb + 3);
        if (ls < lt * D.s || lt < ls * D.s) return 0;
      }
  double mp[3] = {0, 0, 0}, mq[3] = {0, 0, 0};
  for (int k = 0; k < n; ++k) {
    const double* r = pairs + 6 * (int64_t)smp[k];
    for (int c = 0; c < 3; ++c) {
      mp[c] += r[c];
      mq[c] += r[3 + c];
    }
  }
  for (int c = 0; c < 3; ++c) {
    mp[c] /= (double)n;
    mq[c] /= (double)n;
  }
  double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, R[9];
  for (int k = 0; k < n; ++k) {
    const double* r = pairs + 6 * (int64_t)smp[k];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) H[3 * a + b] += (r[a] - mp[a]) * (r[3 + b] - mq[b]);
  }
  svd_rot3(H, R);
  for (int a = 0; a < 3; ++a) {
    T[4 * a] = R[3 * a];
    T[4 * a + 1] = R[3 * a + 1];
    T[4 * a + 2] = R[3 * a + 2];
    T[4 * a + 3] = mq[a] - ((R[3 * a] * mp[0] + R[3 * a + 1] * mp[1]) + R[3 * a + 2] * mp[2]);
  }
  int flags = RS_FLAG_EDGE;
  if (D.d > 0.0)
    for (int k = 0; k < n; ++k)
      if (sqrt(rs_pair_d2(T, pairs + 6 * (int64_t)smp[k])) > D.d) return flags;
  return flags | RS_FLAG_DIST | RS_FLAG_SCORED;
}

__host__ __device__ inline double rs_rmse(int32_t count, double sum) {
  return count > 0 ? sqrt(sum / (double)count) : 0.0;
}

// Open3D's replacement rule: strictly more inliers, or as many and a strictly smaller RMSE.
__host__ __device__ inline bool rs_better(int32_t count, double rmse, const RsBest& b) {
  return count > b.count || (count == b.count && rmse < b.rmse);
}

}  // namespace thip
