// kernels_features.hip -- the correspondence front-end on gfx950: FPFH descriptors and the mutual
// nearest-neighbour feature matcher, the stage BEFORE the registration hot path.
//
// One set of kernels, segmented over a batch of clouds or feature pairs; features.hip is their host side.  The
// single-cloud calls of the C ABI (teaser_hip_compute_fpfh, teaser_hip_match_features) are batches of one.
//
// Replaces, behind the C ABI (those two and teaser_hip_features_*):
//   * teaser::FPFHEstimation::computeFPFHFeatures (reference teaser/src/fpfh.cc:15-43), which is a
//     pass-through to PCL (NOT in the reference tree): pcl::NormalEstimation with a radius search
//     (features/normal_3d.hpp -> common/centroid.hpp computeMeanAndCovarianceMatrix, float accumulators ->
//     common/eigen.hpp eigen33, closed-form roots -> flipNormalTowardsViewpoint, viewpoint 0,0,0) and
//     pcl::FPFHEstimation (features/fpfh.hpp computePointSPFHSignature / weightPointSPFHSignature,
//     features/pfh_tools.hpp computePairFeatures), neighbours from pcl::search::KdTree::radiusSearch
//     (sorted by distance, squared distances, the query point included);
//   * the nearest-neighbour searches of teaser::Matcher::advancedMatching (reference
//     teaser/src/matcher.cc:117-192: FLANN KDTreeSingleIndex, exact L2 1-NN in 33 dimensions).
//
// Design.  Both PCL stages are "for every point, a SEQUENTIAL float reduction over its radius neighbours
// in order of increasing distance", and 71 000 histogram bins of the reference's fixture are decided by
// floor() of those floats -- so the order and the precision of every operation are part of the contract.
// The kd-trees are replaced by what a GPU is good at: brute-force O(n^2) distance tiles through LDS
// (count pass, exclusive scan, fill pass: exact neighbour lists, no tree, no traversal divergence), a
// per-point bitonic sort of (distance, index) in LDS, and one thread per point for the order-sensitive
// reductions (the same operation sequence as the CPU oracle: results are bit-identical to it).  libm's
// float functions are not portable to the last bit, so acos / atan2 / sin / cos are evaluated from IEEE
// double basic operations in a fixed order (the oracle uses the same formulas).  This file is compiled
// with -ffp-contract=off like the rest of the library: no product-add is fused by the compiler; the ONE place where the
// reference's fixtures need fused multiply-adds -- the covariance accumulators of the normals -- says so explicitly.
#include "internal.h"
#include "fdet_math.h"
#include "features_internal.h"

namespace thip {

namespace {

struct Nbr {
  float d2;
  int32_t idx;
};

// ---- deterministic elementary functions (IEEE double basic operations only, fixed order) ---------
// fdet_atan_d / fdet_atan2_d: fdet_math.h, shared with the Open3D-form FPFH
__device__ float fdet_atan2f(float y, float x) { return (float)fdet_atan2_d((double)y, (double)x); }
__device__ float fdet_acosf(float x) {  // x in [0, 1]
  const double xd = (double)x;
  const double s = __builtin_sqrt((1.0 - xd) * (1.0 + xd));
  return (float)fdet_atan2_d(s, xd);
}
__device__ void fdet_sincosf(float th, float* sn, float* cs) {
  const double t = (double)th, t2 = t * t;
  double s = 0.0, c = 0.0;
#pragma unroll 1
  for (int k = 12; k >= 1; --k) {
    s = 1.0 - t2 * s / (double)((2 * k) * (2 * k + 1));
    c = 1.0 - t2 * c / (double)((2 * k - 1) * (2 * k));
  }
  *sn = (float)(t * s);
  *cs = (float)c;
}

// squared distance exactly as flann::L2_Simple<float> accumulates it over x, y, z
__device__ __forceinline__ float feat_d2(float qx, float qy, float qz, float x, float y, float z) {
  const float dx = x - qx, dy = y - qy, dz = z - qz;
  float d2 = dx * dx;
  d2 += dy * dy;
  d2 += dz * dz;
  return d2;
}

// ---- radius neighbour lists: count pass / fill pass over LDS tiles of the cloud ------------------
// grid (blocks of 64 queries, chunks of kFeatChunk data points): a wave owns 64 queries and one chunk, so that a
// 5 000-point cloud is 800 waves (the first version's 20 workgroups left 236 of the 256 CUs idle: 0.39 ms for
// 25 M distance evaluations).  The lists are SORTED by (d2, idx) afterwards (feat_sort_kernel), so the chunks
// may append in any order: the count pass adds into counts[q], the fill pass reserves its run of the list with
// one atomic per (query, chunk).
constexpr int kFeatChunk = 512;

// FILL == 0: counts[q] += |{ i in chunk : d2(q, i) < r2 }| (counts zeroed by the launcher);
// FILL == 1: the chunk's neighbours (d2, i) into list[offset[q] + cursor[q] ...] (cursor zeroed by the launcher)
// (the body of one workgroup: query block `qblock`, data chunk `chunk` of ONE cloud, whose own pointers the kernel
// hands it)
template <int FILL>
__device__ __forceinline__ void feat_radius_block(const float* __restrict__ pts, int n, float r2,
                                                  int32_t* __restrict__ counts, const int64_t* __restrict__ offsets,
                                                  Nbr* __restrict__ list, int qblock, int chunk) {
  __shared__ float tile[kFeatChunk * 3];
  const int q = qblock * 64 + threadIdx.x;
  const bool live = q < n;
  const float qx = live ? pts[3 * q] : 0.f, qy = live ? pts[3 * q + 1] : 0.f, qz = live ? pts[3 * q + 2] : 0.f;
  const int base = chunk * kFeatChunk;
  const int m = min(kFeatChunk, n - base);
  for (int k = threadIdx.x; k < 3 * m; k += 64) tile[k] = pts[3 * base + k];
  __syncthreads();
  if (!live) return;
  int cnt = 0;
#pragma unroll 4
  for (int k = 0; k < m; ++k) cnt += feat_d2(qx, qy, qz, tile[3 * k], tile[3 * k + 1], tile[3 * k + 2]) < r2 ? 1 : 0;
  if (cnt == 0) return;
  const int pos = atomicAdd(&counts[q], cnt);
  if (!FILL) return;
  Nbr* out = list + offsets[q] + pos;
  int c = 0;
  for (int k = 0; k < m; ++k) {
    const float d2 = feat_d2(qx, qy, qz, tile[3 * k], tile[3 * k + 1], tile[3 * k + 2]);
    if (d2 < r2) {
      out[c].d2 = d2;
      out[c].idx = base + k;
      ++c;
    }
  }
}

// exclusive scan of the counts (one workgroup; n <= a few million) + the largest count
// (one workgroup's scan of one cloud)
__device__ __forceinline__ void feat_scan_block(const int32_t* __restrict__ counts, int n,
                                                int64_t* __restrict__ offsets,
                                                int64_t* __restrict__ total_and_max) {
  __shared__ long long part[1024];
  __shared__ int pmax[1024];
  const int t = threadIdx.x;
  const int per = (n + 1023) / 1024;
  const int b = t * per, e = min(n, b + per);
  long long s = 0;
  int mx = 0;
  for (int i = b; i < e; ++i) {
    s += counts[i];
    mx = max(mx, counts[i]);
  }
  part[t] = s;
  pmax[t] = mx;
  __syncthreads();
  if (t == 0) {
    long long acc = 0;
    int m = 0;
    for (int k = 0; k < 1024; ++k) {
      const long long v = part[k];
      part[k] = acc;
      acc += v;
      m = max(m, pmax[k]);
    }
    total_and_max[0] = acc;
    total_and_max[1] = m;
  }
  __syncthreads();
  long long acc = part[t];
  for (int i = b; i < e; ++i) {
    offsets[i] = acc;
    acc += counts[i];
  }
}

// per point: bitonic sort of its list by (d2, idx) in LDS (one 256-thread workgroup per point)
constexpr int kFeatSortCap = 4096;
__device__ __forceinline__ bool nbr_less(const Nbr& a, const Nbr& b) {
  return a.d2 < b.d2 || (a.d2 == b.d2 && a.idx < b.idx);
}
__global__ __launch_bounds__(256) void feat_sort_kernel(const int64_t* __restrict__ offsets,
                                                        const int32_t* __restrict__ counts,
                                                        Nbr* __restrict__ list) {
  __shared__ Nbr buf[kFeatSortCap];
  const int q = blockIdx.x;
  const int k = counts[q];
  if (k <= 1 || k > kFeatSortCap) return;  // (longer lists: feat_sort_long_kernel)
  Nbr* mine = list + offsets[q];
  int P2 = 2;
  while (P2 < k) P2 <<= 1;
  for (int i = threadIdx.x; i < P2; i += 256) {
    if (i < k) {
      buf[i] = mine[i];
    } else {
      buf[i].d2 = __builtin_inff();
      buf[i].idx = 0x7fffffff;
    }
  }
  __syncthreads();
  for (int size = 2; size <= P2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < P2; i += 256) {
        const int l = i ^ stride;
        if (l > i) {
          const bool up = (i & size) == 0;
          const Nbr a = buf[i], b = buf[l];
          if (nbr_less(b, a) == up) {
            buf[i] = b;
            buf[l] = a;
          }
        }
      }
      __syncthreads();
    }
  for (int i = threadIdx.x; i < k; i += 256) mine[i] = buf[i];
}

// Lists longer than the LDS sort holds (a radius that catches more than kFeatSortCap neighbours: dense clouds, large
// radii -- rare at the reference's settings, where a point has a few hundred): rank sort through a scratch copy, one
// workgroup per such list, O(k^2) comparisons.  (d2, idx) is a total order, so the result is the one the LDS sort
// gives; feat_sort_kernel skips these lists.
__global__ __launch_bounds__(256) void feat_sort_long_kernel(const int64_t* __restrict__ offsets,
                                                             const int32_t* __restrict__ counts, Nbr* __restrict__ list,
                                                             Nbr* __restrict__ scratch) {
  const int q = blockIdx.x;
  const int k = counts[q];
  if (k <= kFeatSortCap) return;
  Nbr* mine = list + offsets[q];
  Nbr* out = scratch + offsets[q];
  for (int i = threadIdx.x; i < k; i += 256) {
    const Nbr a = mine[i];
    int rank = 0;
    for (int j = 0; j < k; ++j) rank += nbr_less(mine[j], a) ? 1 : 0;
    out[rank] = a;
  }
  __threadfence_block();
  __syncthreads();
  for (int i = threadIdx.x; i < k; i += 256) mine[i] = out[i];
}

// ---- normals: pcl::NormalEstimation::computeFeature ----------------------------------------------
__device__ void feat_roots2(float b, float c, float* r) {  // pcl::computeRoots2
  r[0] = 0.0f;
  float d = b * b - 4.0f * c;
  if (d < 0.0f) d = 0.0f;
  const float sd = __builtin_sqrtf(d);
  r[2] = 0.5f * (b + sd);
  r[1] = 0.5f * (b - sd);
}
__device__ void feat_roots3(const float* m, float* r) {  // pcl::computeRoots, Scalar = float
  const float m00 = m[0], m01 = m[1], m02 = m[2], m11 = m[4], m12 = m[5], m22 = m[8];
  const float c0 = m00 * m11 * m22 + 2.0f * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01;
  const float c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12;
  const float c2 = m00 + m11 + m22;
  if (__builtin_fabsf(c0) < 1.1920929e-07f) {
    feat_roots2(c2, c1, r);
    return;
  }
  const float s_inv3 = 1.0f / 3.0f, s_sqrt3 = __builtin_sqrtf(3.0f);
  const float c2_over_3 = c2 * s_inv3;
  float a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
  if (a_over_3 > 0.0f) a_over_3 = 0.0f;
  const float half_b = 0.5f * (c0 + c2_over_3 * (2.0f * c2_over_3 * c2_over_3 - c1));
  float q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
  if (q > 0.0f) q = 0.0f;
  const float rho = __builtin_sqrtf(-a_over_3);
  const float theta = fdet_atan2f(__builtin_sqrtf(-q), half_b) * s_inv3;
  float cos_theta, sin_theta;
  fdet_sincosf(theta, &sin_theta, &cos_theta);
  r[0] = c2_over_3 + 2.0f * rho * cos_theta;
  r[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
  r[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
  float t;
  if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
  if (r[1] >= r[2]) {
    t = r[1]; r[1] = r[2]; r[2] = t;
    if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
  }
  if (r[0] <= 0.0f) feat_roots2(c2, c1, r);
}
__device__ __forceinline__ void feat_cross(const float* a, const float* b, float* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// (the normal of point q of one cloud: one thread; every pointer is that cloud's own)
__device__ __forceinline__ void feat_normal_point(const float* __restrict__ pts, int q,
                                                  const int64_t* __restrict__ offsets,
                                                  const int32_t* __restrict__ counts, const Nbr* __restrict__ list,
                                                  float* __restrict__ normals) {
  const int k = counts[q];
  float* out = normals + 3 * q;
  if (k < 3) {  // computePointNormal: too few neighbours
    out[0] = out[1] = out[2] = __builtin_nanf("");
    return;
  }
  const Nbr* nb = list + offsets[q];
  // computeMeanAndCovarianceMatrix: nine float accumulators over the RAW coordinates, in list order,
  float acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int j = 0; j < k; ++j) {
    const int i = nb[j].idx;
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    // FUSED multiply-adds, as an FMA-contracting (-march=native) build of the reference compiles PCL's
    // `accu[k] += p.a * p.b` -- the form the reference's fixtures were generated with (oracle/features_oracle.c,
    // feat_estimate_normals form 0: the matcher fixture's 189 pairs depend on it)
    acc[0] = __builtin_fmaf(x, x, acc[0]); acc[1] = __builtin_fmaf(x, y, acc[1]); acc[2] = __builtin_fmaf(x, z, acc[2]);
    acc[3] = __builtin_fmaf(y, y, acc[3]); acc[4] = __builtin_fmaf(y, z, acc[4]); acc[5] = __builtin_fmaf(z, z, acc[5]);
    acc[6] += x; acc[7] += y; acc[8] += z;
  }
  for (int i = 0; i < 9; ++i) acc[i] /= (float)k;
  float cov[9];
  cov[0] = __builtin_fmaf(-acc[6], acc[6], acc[0]);  // (`accu[k] - accu[6] * accu[6]`, fused likewise)
  cov[1] = __builtin_fmaf(-acc[6], acc[7], acc[1]);
  cov[2] = __builtin_fmaf(-acc[6], acc[8], acc[2]);
  cov[4] = __builtin_fmaf(-acc[7], acc[7], acc[3]);
  cov[5] = __builtin_fmaf(-acc[7], acc[8], acc[4]);
  cov[8] = __builtin_fmaf(-acc[8], acc[8], acc[5]);
  cov[3] = cov[1];
  cov[6] = cov[2];
  cov[7] = cov[5];
  // pcl::eigen33 (smallest eigenvalue and its eigenvector)
  float scale = 0.0f;
  for (int i = 0; i < 9; ++i) scale = __builtin_fmaxf(scale, __builtin_fabsf(cov[i]));
  if (scale <= 1.17549435e-38f) scale = 1.0f;
  float m[9];
  for (int i = 0; i < 9; ++i) m[i] = cov[i] / scale;
  float r[3];
  feat_roots3(m, r);
  m[0] -= r[0];
  m[4] -= r[0];
  m[8] -= r[0];
  float v1[3], v2[3], v3[3];
  feat_cross(m, m + 3, v1);
  feat_cross(m, m + 6, v2);
  feat_cross(m + 3, m + 6, v3);
  const float l1 = v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2];
  const float l2 = v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2];
  const float l3 = v3[0] * v3[0] + v3[1] * v3[1] + v3[2] * v3[2];
  float nv[3], l;
  if (l1 >= l2 && l1 >= l3) { nv[0] = v1[0]; nv[1] = v1[1]; nv[2] = v1[2]; l = l1; }
  else if (l2 >= l1 && l2 >= l3) { nv[0] = v2[0]; nv[1] = v2[1]; nv[2] = v2[2]; l = l2; }
  else { nv[0] = v3[0]; nv[1] = v3[1]; nv[2] = v3[2]; l = l3; }
  const float s = __builtin_sqrtf(l);
  nv[0] /= s;
  nv[1] /= s;
  nv[2] /= s;
  // flipNormalTowardsViewpoint, viewpoint (0, 0, 0)
  const float vx = 0.0f - pts[3 * q], vy = 0.0f - pts[3 * q + 1], vz = 0.0f - pts[3 * q + 2];
  const float cos_theta = vx * nv[0] + vy * nv[1] + vz * nv[2];
  if (cos_theta < 0) {
    nv[0] *= -1;
    nv[1] *= -1;
    nv[2] *= -1;
  }
  out[0] = nv[0];
  out[1] = nv[1];
  out[2] = nv[2];
}

// ---- SPFH / FPFH -----------------------------------------------------------------------------------
// Eigen::Vector4f dot with a zero 4th component, in the order Eigen's SSE reduction adds the lane products
__device__ __forceinline__ float feat_dot4(const float* x, const float* y) {
  const float p0 = x[0] * y[0], p1 = x[1] * y[1], p2 = x[2] * y[2];
  return (p0 + p2) + (p1 + 0.0f);
}
__device__ bool feat_pair_features(const float* p1, const float* n1, const float* p2, const float* n2, float* f) {
  float dp[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  const float f4 = __builtin_sqrtf(feat_dot4(dp, dp));
  if (f4 == 0.0f) return false;
  float a[3] = {n1[0], n1[1], n1[2]}, b[3] = {n2[0], n2[1], n2[2]};
  const float angle1 = feat_dot4(a, dp) / f4;
  const float angle2 = feat_dot4(b, dp) / f4;
  float f3;
  if (fdet_acosf(__builtin_fabsf(angle1)) > fdet_acosf(__builtin_fabsf(angle2))) {  // switch p1 and p2
    for (int i = 0; i < 3; ++i) {
      a[i] = n2[i];
      b[i] = n1[i];
      dp[i] *= -1;
    }
    f3 = -angle2;
  } else {
    f3 = angle1;
  }
  float v[3];
  feat_cross(dp, a, v);
  const float vn = __builtin_sqrtf(feat_dot4(v, v));
  if (vn == 0.0f) return false;
  v[0] /= vn;
  v[1] /= vn;
  v[2] /= vn;
  float w[3];
  feat_cross(a, v, w);
  f[1] = feat_dot4(v, b);
  f[0] = fdet_atan2f(feat_dot4(w, b), feat_dot4(a, b));
  f[2] = f3;
  f[3] = f4;
  return true;
}
// static_cast<int>(std::floor(x)) with the x86 result for NaN (INT_MIN -> clamped to bin 0)
__device__ __forceinline__ int feat_bin(double x) {
  if (!(x == x)) return 0;
  const double fl = __builtin_floor(x);
  int hi = fl < 0.0 ? 0 : (fl >= 11.0 ? 10 : (int)fl);
  return hi;
}

// computePointSPFHSignature: one WAVE per point, its lanes over the neighbours.  Every contributing pair adds
// the SAME float (incr) to one bin of each of the three histograms, so a bin's value is incr added count times
// in float -- whatever the order of the neighbours: the lanes count into LDS, then lane b replays the additions
// of bin b.  (One thread per point, the first version, was 79 waves on 1 024 SIMDs and 1.98 ms at n = 5 000.)
// (wave w of the workgroup computes point p of one cloud -- or nothing when !live; the four waves of a workgroup may
// serve different clouds, each with that cloud's own pointers.  Every wave reaches both barriers.)
__device__ __forceinline__ void feat_spfh_point(const float* __restrict__ pts, const float* __restrict__ normals,
                                                bool live, int p, const int64_t* __restrict__ offsets,
                                                const int32_t* __restrict__ counts, const Nbr* __restrict__ list,
                                                float* __restrict__ spfh) {
  __shared__ int bins[4][33];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (lane < 33) bins[w][lane] = 0;
  __syncthreads();
  const int k = live ? counts[p] : 0;
  if (live) {
    const Nbr* nb = list + offsets[p];
    const float d_pi = 1.0f / (2.0f * 3.14159274101257324f);  // 1.0f / (2.0f * static_cast<float>(M_PI))
    const double pi = 3.14159265358979323846;
    const float P[3] = {pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]};
    const float N[3] = {normals[3 * p], normals[3 * p + 1], normals[3 * p + 2]};
    for (int j = lane; j < k; j += 64) {
      const int qi = nb[j].idx;
      if (qi == p) continue;
      const float Q[3] = {pts[3 * qi], pts[3 * qi + 1], pts[3 * qi + 2]};
      const float M[3] = {normals[3 * qi], normals[3 * qi + 1], normals[3 * qi + 2]};
      float f[4];
      if (!feat_pair_features(P, N, Q, M, f)) continue;
      atomicAdd(&bins[w][feat_bin(11 * (((double)f[0] + pi) * (double)d_pi))], 1);
      atomicAdd(&bins[w][11 + feat_bin(11 * (((double)f[1] + 1.0) * 0.5))], 1);
      atomicAdd(&bins[w][22 + feat_bin(11 * (((double)f[2] + 1.0) * 0.5))], 1);
    }
  }
  __syncthreads();
  if (live && lane < 33) {
    const float incr = 100.0f / (float)(k - 1);
    const int c = bins[w][lane];
    float h = 0.0f;
    for (int i = 0; i < c; ++i) h += incr;
    spfh[(size_t)p * 33 + lane] = h;
  }
}

// weightPointSPFHSignature: one wave per point, lane b = bin b; the neighbours in order of increasing distance
// (the float sums depend on it).  Per neighbour the bin values val_b = spfh[b] * weight are one coalesced row;
// the group sums add them in the reference's order (j outer, bin inner), every lane of a group carrying its
// group's running sum and fetching the eleven addends across the lanes.  A skipped neighbour (d2 == 0)
// contributes +0, which leaves the non-negative sums unchanged bit for bit.  Neighbour records are wave-uniform
// (scalar loads), fetched one block of kFpfhBlock ahead of the rows they index.
constexpr int kFpfhBlock = 8;
// (one wave: point p of one cloud, with that cloud's own pointers)
__device__ __forceinline__ void feat_fpfh_point(int p, const int64_t* __restrict__ offsets,
                                                const int32_t* __restrict__ counts, const Nbr* __restrict__ list,
                                                const float* __restrict__ spfh, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int k = counts[p];
  const Nbr* nb = list + offsets[p];
  const int b = lane < 33 ? lane : 32;  // (lanes 33 .. 63 shadow bin 32; they do not store)
  const int g0 = 11 * (b / 11);
  float o = 0.0f, sum = 0.0f;
  Nbr cur[kFpfhBlock], nxt[kFpfhBlock];
#pragma unroll
  for (int u = 0; u < kFpfhBlock; ++u) {
    cur[u].d2 = u < k ? nb[u].d2 : 0.0f;
    cur[u].idx = u < k ? nb[u].idx : p;
  }
  for (int j0 = 0; j0 < k; j0 += kFpfhBlock) {
    float hv[kFpfhBlock];
#pragma unroll
    for (int u = 0; u < kFpfhBlock; ++u) hv[u] = spfh[(size_t)cur[u].idx * 33 + b];
#pragma unroll
    for (int u = 0; u < kFpfhBlock; ++u) {
      const int j = j0 + kFpfhBlock + u;
      nxt[u].d2 = j < k ? nb[j].d2 : 0.0f;
      nxt[u].idx = j < k ? nb[j].idx : p;
    }
#pragma unroll
    for (int u = 0; u < kFpfhBlock; ++u) {
      const float d2 = cur[u].d2;
      const float weight = 1.0f / d2;
      const float val = d2 == 0.0f ? 0.0f : hv[u] * weight;
      o += val;
#pragma unroll
      for (int i = 0; i < 11; ++i) sum += __shfl(val, g0 + i);
    }
#pragma unroll
    for (int u = 0; u < kFpfhBlock; ++u) cur[u] = nxt[u];
  }
  if (sum != 0) sum = 100.0f / sum;
  if (lane < 33) out[(size_t)p * 33 + lane] = o * sum;
}

// ---- exact L2 k-NN in `dim` dimensions (include/teaser_hip.h, "k nearest"): the k smallest (d, index) per query ------
// K = 1 is the matcher's two searches.
// grid (query blocks of 64, data chunks of kNnChunk): a thread owns one query, walks the chunk's data points through
// an LDS tile, accumulating (q_c - d_c)^2 over c in order in float, and keeps the K best of its chunk as a list sorted
// by (d, index) in registers.
// Exact L2, brute force.  The arithmetic of one distance is fixed by the oracle (flann::L2<float> order:
// d += (q_c - x_c)^2 for c = 0 .. dim-1, float), so the speed has to come from the layout: the query vector of a
// thread lives in REGISTERS (dim is a template parameter for the 33-bin FPFH signature; other dims take the generic
// instantiation with the query in LDS, one row per thread), a tile of kNnTile data points is staged in LDS and read
// back as broadcast ds_read_b128, and the data set is cut into chunks of kNnChunk points so that a 5 000 x 5 000 match
// fills the GPU (1 700 waves instead of the 164 of the first version, which took 6 ms per direction -- 0.3 TFLOP/s).
// K is a template parameter (1, 2, 4, 8, 16; a call's k is rounded up): the list is only ever indexed by the unrolled
// loops' constants, so it stays in VGPRs -- a runtime-indexed array would live in scratch memory.  Candidates arrive
// in ascending index order and the comparisons are strict, so among equal d the lower index stays ahead (K = 1: the
// first strict minimum); NaN and +inf fail every `<` against the +inf the list starts with and never enter.
constexpr int kNnChunk = 256;
constexpr int kNnTile = 64;
constexpr int kNnMaxDim = 64;
template <int K>
__device__ __forceinline__ void feat_knn_insert(float (&ld)[K], int32_t (&li)[K], float d, int32_t idx) {
#pragma unroll
  for (int s = K - 1; s > 0; --s) {  // (downwards: slot s - 1 is still the old one when slot s takes it)
    const bool shift = d < ld[s - 1], here = d < ld[s];
    li[s] = shift ? li[s - 1] : (here ? idx : li[s]);
    ld[s] = shift ? ld[s - 1] : (here ? d : ld[s]);
  }
  li[0] = d < ld[0] ? idx : li[0];
  ld[0] = d < ld[0] ? d : ld[0];
}
// (the body of one workgroup: query block `qblock` against data chunk `chunk` of ONE search)
// partials: [chunk][slot][query], so that the lanes of a wave store neighbouring words
template <int DIM, int K>
__device__ __forceinline__ void feat_knn_partial_block(const float* __restrict__ data, int nd,
                                                       const float* __restrict__ query, int nq, int dim_rt,
                                                       float* __restrict__ part_d, int32_t* __restrict__ part_i,
                                                       int qblock, int chunk) {
  constexpr int kPad = DIM > 0 ? ((DIM + 3) & ~3) : kNnMaxDim;  // floats per staged point (16-byte rows)
  __shared__ __attribute__((aligned(16))) float tile[kNnTile * kPad];
  __shared__ float qs[DIM > 0 ? 1 : 64 * (kNnMaxDim + 1)];
  const int dim = DIM > 0 ? DIM : dim_rt;
  const int q = qblock * 64 + threadIdx.x;
  const bool live = q < nq;
  float qr[DIM > 0 ? kPad : 1];
  if (DIM > 0) {
#pragma unroll
    for (int c = 0; c < kPad; ++c) qr[c] = (live && c < DIM) ? query[(size_t)q * DIM + c] : 0.f;
  } else {
    for (int c = 0; c < dim; ++c) qs[threadIdx.x * (kNnMaxDim + 1) + c] = live ? query[(size_t)q * dim + c] : 0.f;
  }
  const int lo = chunk * kNnChunk, hi = min(nd, lo + kNnChunk);
  float ld[K];
  int32_t li[K];
#pragma unroll
  for (int s = 0; s < K; ++s) {
    ld[s] = __builtin_inff();
    li[s] = -1;
  }
  for (int base = lo; base < hi; base += kNnTile) {
    const int m = min(kNnTile, hi - base);
    __syncthreads();
    if (DIM > 0) {
      for (int k = threadIdx.x; k < m * kPad; k += 64) {
        const int pt = k / kPad, c = k - pt * kPad;
        tile[k] = c < DIM ? data[(size_t)(base + pt) * DIM + c] : 0.f;
      }
    } else {
      for (int k = threadIdx.x; k < m * dim; k += 64) tile[(k / dim) * kPad + (k % dim)] = data[(size_t)base * dim + k];
    }
    __syncthreads();
    for (int k = 0; k < m; ++k) {
      float d = 0;
      if (DIM > 0) {
        const float4* row = reinterpret_cast<const float4*>(tile + k * kPad);
#pragma unroll
        for (int c4 = 0; c4 < kPad / 4; ++c4) {
          const float4 x = row[c4];  // broadcast: every lane reads the same 16 bytes
          const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (4 * c4 + e < DIM) {  // (the padding is skipped: d + 0 * 0 would still be a float operation)
              const float t = qr[4 * c4 + e] - xs[e];
              d += t * t;
            }
        }
      } else {
        for (int c = 0; c < dim; ++c) {
          const float t = qs[threadIdx.x * (kNnMaxDim + 1) + c] - tile[k * kPad + c];
          d += t * t;
        }
      }
      if (d < ld[K - 1]) feat_knn_insert<K>(ld, li, d, base + k);  // one compare per distance in the common case
    }
  }
  if (live) {
#pragma unroll
    for (int s = 0; s < K; ++s) {
      part_d[((size_t)chunk * K + s) * nq + q] = ld[s];
      part_i[((size_t)chunk * K + s) * nq + q] = li[s];
    }
  }
}
// One thread per query: the chunks' lists, taken in chunk order and slot order, go through the same strict insertion,
// so an entry of a lower chunk (lower indices) stays ahead of an equal d of a higher one: the global (d, index) order.
// A chunk's list is sorted, so its first entry that does not enter ends that chunk.  Row q of idx / dist: k slots.
template <int K>
__device__ __forceinline__ void feat_knn_final_query(const float* __restrict__ part_d,
                                                     const int32_t* __restrict__ part_i, int nq, int chunks, int k,
                                                     int32_t* __restrict__ idx, float* __restrict__ dist, int q) {
  float ld[K];
  int32_t li[K];
#pragma unroll
  for (int s = 0; s < K; ++s) {
    ld[s] = __builtin_inff();
    li[s] = -1;
  }
  for (int c = 0; c < chunks; ++c)
    for (int s = 0; s < K; ++s) {
      const float d = part_d[((size_t)c * K + s) * nq + q];
      if (!(d < ld[K - 1])) break;
      feat_knn_insert<K>(ld, li, d, part_i[((size_t)c * K + s) * nq + q]);
    }
#pragma unroll
  for (int s = 0; s < K; ++s)
    if (s < k) {
      idx[(size_t)q * k + s] = li[s];
      if (dist) dist[(size_t)q * k + s] = ld[s];
    }
}

}  // namespace

// ---- the kernels: one launch for many clouds (or searches) -------------------------------------------------------
// A block finds its cloud (or search) through a host-built block -> problem map and the descriptor table, then runs
// the body above with that problem's own pointers: the chunking of a cloud depends on that cloud alone, so what is
// computed for it -- and, after the (d2, idx) sort, in which order -- does not depend on its neighbours in the batch.
// One cloud or one pair is a batch of one.
namespace {

template <int FILL>
__global__ __launch_bounds__(64) void feat_radius_batch_kernel(const FeatCloudDesc* __restrict__ desc,
                                                               const int32_t* __restrict__ blk_cloud, int blk_base,
                                                               int which, const float* __restrict__ pts,
                                                               int32_t* __restrict__ counts,
                                                               const int64_t* __restrict__ offsets,
                                                               Nbr* __restrict__ list) {
  const int blk = blk_base + (int)blockIdx.x;
  const FeatCloudDesc d = desc[blk_cloud[blk]];
  const int local = blk - d.blk_off;
  const int chunk = local / d.qblocks, qblock = local - chunk * d.qblocks;
  feat_radius_block<FILL>(pts + 3 * d.off, d.n, d.r2[which], counts + d.off, FILL ? offsets + d.off : nullptr, list,
                          qblock, chunk);
}

// one workgroup per cloud
__global__ __launch_bounds__(1024) void feat_scan_batch_kernel(const FeatCloudDesc* __restrict__ desc,
                                                               const int32_t* __restrict__ counts,
                                                               int64_t* __restrict__ offsets,
                                                               int64_t* __restrict__ meta) {
  const FeatCloudDesc d = desc[blockIdx.x];
  feat_scan_block(counts + d.off, d.n, offsets + d.off, meta + 2 * (size_t)blockIdx.x);
}

__global__ __launch_bounds__(256) void feat_rebase_kernel(const int32_t* __restrict__ pt_cloud,
                                                          const int64_t* __restrict__ base, int64_t n_pts,
                                                          int64_t* __restrict__ offsets) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g < n_pts) offsets[g] += base[pt_cloud[g]];
}

__global__ __launch_bounds__(128) void feat_normals_batch_kernel(const FeatCloudDesc* __restrict__ desc,
                                                                 const int32_t* __restrict__ pt_cloud, int64_t pt0,
                                                                 int64_t pt1, const float* __restrict__ pts,
                                                                 const int64_t* __restrict__ offsets,
                                                                 const int32_t* __restrict__ counts,
                                                                 const Nbr* __restrict__ list,
                                                                 float* __restrict__ normals) {
  const int64_t g = pt0 + (int64_t)blockIdx.x * 128 + threadIdx.x;
  if (g >= pt1) return;
  const int64_t off = desc[pt_cloud[g]].off;
  feat_normal_point(pts + 3 * off, (int)(g - off), offsets + off, counts + off, list, normals + 3 * off);
}

__global__ __launch_bounds__(256) void feat_spfh_batch_kernel(const FeatCloudDesc* __restrict__ desc,
                                                              const int32_t* __restrict__ pt_cloud, int64_t pt0,
                                                              int64_t pt1, const float* __restrict__ pts,
                                                              const float* __restrict__ normals,
                                                              const int64_t* __restrict__ offsets,
                                                              const int32_t* __restrict__ counts,
                                                              const Nbr* __restrict__ list, float* __restrict__ spfh) {
  const int64_t g = pt0 + (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool live = g < pt1;
  const int64_t off = live ? desc[pt_cloud[g]].off : 0;
  feat_spfh_point(pts + 3 * off, normals + 3 * off, live, (int)(g - off), offsets + off, counts + off, list,
                  spfh + 33 * off);
}

__global__ __launch_bounds__(256) void feat_fpfh_batch_kernel(const FeatCloudDesc* __restrict__ desc,
                                                              const int32_t* __restrict__ pt_cloud, int64_t pt0,
                                                              int64_t pt1, const int64_t* __restrict__ offsets,
                                                              const int32_t* __restrict__ counts,
                                                              const Nbr* __restrict__ list,
                                                              const float* __restrict__ spfh, float* __restrict__ out) {
  const int64_t g = pt0 + (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (g >= pt1) return;
  const int64_t off = desc[pt_cloud[g]].off;
  feat_fpfh_point((int)(g - off), offsets + off, counts + off, list, spfh + 33 * off, out + 33 * off);
}

// k-NN searches: part_off counts the (chunk, slot, query) partial entries and nn_off the nq x k result slots of the
// searches before this one.
template <int DIM, int K>
__global__ __launch_bounds__(64) void feat_knn_partial_batch_kernel(const FeatSearchDesc* __restrict__ search,
                                                                    const int32_t* __restrict__ blk_search,
                                                                    int blk_base, const float* __restrict__ feat,
                                                                    int dim_rt, float* __restrict__ part_d,
                                                                    int32_t* __restrict__ part_i) {
  const int blk = blk_base + (int)blockIdx.x;
  const FeatSearchDesc d = search[blk_search[blk]];
  const int local = blk - d.blk_off;
  const int chunk = local / d.qblocks, qblock = local - chunk * d.qblocks;
  const int dim = DIM > 0 ? DIM : dim_rt;
  feat_knn_partial_block<DIM, K>(feat + d.data_row * dim, d.nd, feat + d.query_row * dim, d.nq, dim_rt,
                                 part_d + d.part_off, part_i + d.part_off, qblock, chunk);
}
// grid (query blocks of 256 of the largest search, searches)
template <int K>
__global__ __launch_bounds__(256) void feat_knn_final_batch_kernel(const FeatSearchDesc* __restrict__ search, int s0,
                                                                   const float* __restrict__ part_d,
                                                                   const int32_t* __restrict__ part_i, int k,
                                                                   int32_t* __restrict__ idx,
                                                                   float* __restrict__ dist) {
  const FeatSearchDesc d = search[s0 + (int)blockIdx.y];
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= d.nq) return;
  feat_knn_final_query<K>(part_d + d.part_off, part_i + d.part_off, d.nq, (d.nd + kNnChunk - 1) / kNnChunk, k,
                          idx + d.nn_off, dist ? dist + d.nn_off : nullptr, q);
}
// Searches 2 p (forward: rows F[i] of source row i) and 2 p + 1 (backward: rows B[j] of target row j) of pair
// p0 + blockIdx.y; one thread per forward entry e = i * k + slot: keep[e] = whether i is in B[F[i][slot]].
__global__ __launch_bounds__(256) void feat_knn_mutual_batch_kernel(const FeatSearchDesc* __restrict__ search, int p0,
                                                                    int k, const int32_t* __restrict__ idx,
                                                                    uint8_t* __restrict__ keep) {
  const int p = p0 + (int)blockIdx.y;
  const FeatSearchDesc f = search[2 * p], b = search[2 * p + 1];
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)f.nq * k) return;
  const int i = (int)(e / k);
  const int j = idx[f.nn_off + e];
  bool found = false;
  if (j >= 0 && j < b.nq)
    for (int s = 0; s < k; ++s) found |= idx[b.nn_off + (int64_t)j * k + s] == i;
  keep[f.nn_off + e] = found ? 1 : 0;
}

// The matcher's tuple constraint (include/teaser_hip.h, "tuple_test_batch"): trial i of a problem is a function of
// (seed, i) alone -- splitmix64's state after m draws is seed + m gamma -- so one lane takes one trial and strides over
// the problem's trials with the problem's own blocks.  The arithmetic is teaser_hip_tuple_test's, operation by
// operation: the exact 64-bit remainder, float differences, squares summed in x, y, z order (no contraction: the
// Makefile's -ffp-contract=off), the correctly rounded sqrt and division hipcc emits for the plain operators.  A
// passing trial raises the keep flag of its three correspondences; every writer writes 1, so plain byte stores do,
// and a flag that is already up is not written again.  The six points and three pairs of a trial are gathered
// straight from global memory: a problem's clouds and pairs are a few hundred KiB, which the L2 holds.
constexpr int kTupleMaxBlocks = 2048;  // blocks of one problem: 8 per CU, the rest of its trials by the grid stride
__device__ __forceinline__ uint64_t feat_tuple_draw(uint64_t seed, uint64_t m) {
  uint64_t z = seed + m * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ float feat_tuple_dist(const float* __restrict__ p, int a, int b) {
  const float dx = p[3 * (int64_t)a] - p[3 * (int64_t)b], dy = p[3 * (int64_t)a + 1] - p[3 * (int64_t)b + 1],
              dz = p[3 * (int64_t)a + 2] - p[3 * (int64_t)b + 2];
  return sqrtf(dx * dx + dy * dy + dz * dz);
}
__global__ __launch_bounds__(256) void feat_tuple_batch_kernel(const FeatTupleDesc* __restrict__ desc,
                                                               const int32_t* __restrict__ blk_problem, int blk_base,
                                                               const float* __restrict__ pts,
                                                               const int2* __restrict__ pairs,
                                                               uint8_t* __restrict__ keep) {
  const int blk = blk_base + (int)blockIdx.x;
  const FeatTupleDesc d = desc[blk_problem[blk]];
  const uint64_t n = (uint64_t)d.ncorr;
  const int64_t trials = 100 * d.ncorr;  // matcher.cc:231
  const int64_t stride = (int64_t)d.n_blk * 256;
  const float* __restrict__ src = pts + 3 * d.src_off;
  const float* __restrict__ dst = pts + 3 * d.dst_off;
  const int2* __restrict__ pr = pairs + d.pair_off;
  uint8_t* __restrict__ flag = keep + d.pair_off;
  const float scale = d.scale;
  for (int64_t i = (int64_t)(blk - d.blk_off) * 256 + threadIdx.x; i < trials; i += stride) {
    const uint64_t m = 3 * (uint64_t)i;
    const uint64_t r0 = feat_tuple_draw(d.seed, m + 1) % n, r1 = feat_tuple_draw(d.seed, m + 2) % n,
                   r2 = feat_tuple_draw(d.seed, m + 3) % n;
    const int2 c0 = pr[r0], c1 = pr[r1], c2 = pr[r2];  // (.x, .y) = (source index, target index)
    const float li0 = feat_tuple_dist(src, c0.x, c1.x), li1 = feat_tuple_dist(src, c1.x, c2.x),
                li2 = feat_tuple_dist(src, c2.x, c0.x);
    const float lj0 = feat_tuple_dist(dst, c0.y, c1.y), lj1 = feat_tuple_dist(dst, c1.y, c2.y),
                lj2 = feat_tuple_dist(dst, c2.y, c0.y);
    if ((li0 * scale < lj0) && (lj0 < li0 / scale) && (li1 * scale < lj1) && (lj1 < li1 / scale) &&
        (li2 * scale < lj2) && (lj2 < li2 / scale)) {  // matcher.cc:267-268
      if (!flag[r0]) flag[r0] = 1;
      if (!flag[r1]) flag[r1] = 1;
      if (!flag[r2]) flag[r2] = 1;
    }
  }
}

}  // namespace

// ---- launchers and the sizes the host plans with ------------------------------------------------------------------
int feat_radius_chunk() { return kFeatChunk; }
int64_t feat_nbr_bytes() { return (int64_t)sizeof(Nbr); }
int feat_sort_capacity() { return kFeatSortCap; }
int feat_nn_chunks(int nd) { return (nd + kNnChunk - 1) / kNnChunk; }
int feat_nn_max_dim() { return kNnMaxDim; }

void launch_feat_radius_count_batch(hipStream_t s, const FeatCloudDesc* d_desc, const int32_t* d_blk_cloud, int blk_base,
                                    int n_blk, int which, const float* d_pts, int32_t* d_counts) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(feat_radius_batch_kernel<0>, dim3(n_blk), dim3(64), 0, s, d_desc, d_blk_cloud, blk_base, which,
                     d_pts, d_counts, static_cast<const int64_t*>(nullptr), static_cast<Nbr*>(nullptr));
}
void launch_feat_scan_batch(hipStream_t s, const FeatCloudDesc* d_desc, int batch, const int32_t* d_counts,
                            int64_t* d_offsets, int64_t* d_meta) {
  if (batch <= 0) return;
  hipLaunchKernelGGL(feat_scan_batch_kernel, dim3(batch), dim3(1024), 0, s, d_desc, d_counts, d_offsets, d_meta);
}
void launch_feat_rebase(hipStream_t s, const int32_t* d_pt_cloud, const int64_t* d_base, int64_t n_pts,
                        int64_t* d_offsets) {
  if (n_pts <= 0) return;
  hipLaunchKernelGGL(feat_rebase_kernel, dim3((unsigned)((n_pts + 255) / 256)), dim3(256), 0, s, d_pt_cloud, d_base,
                     n_pts, d_offsets);
}
void launch_feat_lists_batch(hipStream_t s, const FeatCloudDesc* d_desc, const int32_t* d_blk_cloud, int blk_base,
                             int n_blk, int which, int64_t pt0, int64_t pt1, const float* d_pts,
                             const int32_t* d_counts, int32_t* d_cursor, const int64_t* d_offsets, void* d_list,
                             void* d_scratch) {
  if (n_blk <= 0 || pt1 <= pt0) return;
  Nbr* list = reinterpret_cast<Nbr*>(d_list);
  hipLaunchKernelGGL(feat_radius_batch_kernel<1>, dim3(n_blk), dim3(64), 0, s, d_desc, d_blk_cloud, blk_base, which,
                     d_pts, d_cursor, d_offsets, list);
  const unsigned n = (unsigned)(pt1 - pt0);  // one workgroup per list, offsets being global
  hipLaunchKernelGGL(feat_sort_kernel, dim3(n), dim3(256), 0, s, d_offsets + pt0, d_counts + pt0, list);
  if (d_scratch)
    hipLaunchKernelGGL(feat_sort_long_kernel, dim3(n), dim3(256), 0, s, d_offsets + pt0, d_counts + pt0, list,
                       reinterpret_cast<Nbr*>(d_scratch));
}
void launch_feat_normals_batch(hipStream_t s, const FeatCloudDesc* d_desc, const int32_t* d_pt_cloud, int64_t pt0,
                               int64_t pt1, const float* d_pts, const int64_t* d_offsets, const int32_t* d_counts,
                               const void* d_list, float* d_normals) {
  if (pt1 <= pt0) return;
  hipLaunchKernelGGL(feat_normals_batch_kernel, dim3((unsigned)((pt1 - pt0 + 127) / 128)), dim3(128), 0, s, d_desc,
                     d_pt_cloud, pt0, pt1, d_pts, d_offsets, d_counts, reinterpret_cast<const Nbr*>(d_list), d_normals);
}
void launch_feat_fpfh_batch(hipStream_t s, const FeatCloudDesc* d_desc, const int32_t* d_pt_cloud, int64_t pt0,
                            int64_t pt1, const float* d_pts, const float* d_normals, const int64_t* d_offsets,
                            const int32_t* d_counts, const void* d_list, float* d_spfh, float* d_out) {
  if (pt1 <= pt0) return;
  const unsigned blocks = (unsigned)((pt1 - pt0 + 3) / 4);
  hipLaunchKernelGGL(feat_spfh_batch_kernel, dim3(blocks), dim3(256), 0, s, d_desc, d_pt_cloud, pt0, pt1, d_pts,
                     d_normals, d_offsets, d_counts, reinterpret_cast<const Nbr*>(d_list), d_spfh);
  hipLaunchKernelGGL(feat_fpfh_batch_kernel, dim3(blocks), dim3(256), 0, s, d_desc, d_pt_cloud, pt0, pt1, d_offsets,
                     d_counts, reinterpret_cast<const Nbr*>(d_list), d_spfh, d_out);
}
int feat_knn_slots(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16; }

namespace {
template <int K>
void launch_feat_knn_slots(hipStream_t s, const FeatSearchDesc* d_search, const int32_t* d_blk_search, int blk_base,
                           int n_blk, int s0, int s1, int max_nq, const float* d_feat, int dim, int k, float* d_part_d,
                           int32_t* d_part_i, int32_t* d_idx, float* d_dist) {
  if (dim == 33)  // pcl::FPFHSignature33
    hipLaunchKernelGGL((feat_knn_partial_batch_kernel<33, K>), dim3(n_blk), dim3(64), 0, s, d_search, d_blk_search,
                       blk_base, d_feat, dim, d_part_d, d_part_i);
  else
    hipLaunchKernelGGL((feat_knn_partial_batch_kernel<0, K>), dim3(n_blk), dim3(64), 0, s, d_search, d_blk_search,
                       blk_base, d_feat, dim, d_part_d, d_part_i);
  for (int y0 = s0; y0 < s1; y0 += 65535)  // (the grid's y extent)
    hipLaunchKernelGGL(feat_knn_final_batch_kernel<K>, dim3((max_nq + 255) / 256, std::min(65535, s1 - y0)), dim3(256),
                       0, s, d_search, y0, d_part_d, d_part_i, k, d_idx, d_dist);
}
}  // namespace

void launch_feat_knn_batch(hipStream_t s, const FeatSearchDesc* d_search, const int32_t* d_blk_search, int blk_base,
                           int n_blk, int s0, int s1, int max_nq, const float* d_feat, int dim, int k, float* d_part_d,
                           int32_t* d_part_i, int32_t* d_idx, float* d_dist) {
  if (n_blk <= 0 || s1 <= s0 || max_nq <= 0) return;
  switch (feat_knn_slots(k)) {
#define THIP_KNN_CASE(K)                                                                                         \
  case K:                                                                                                        \
    launch_feat_knn_slots<K>(s, d_search, d_blk_search, blk_base, n_blk, s0, s1, max_nq, d_feat, dim, k, d_part_d, \
                             d_part_i, d_idx, d_dist);                                                           \
    break;
    THIP_KNN_CASE(1)
    THIP_KNN_CASE(2)
    THIP_KNN_CASE(4)
    THIP_KNN_CASE(8)
    THIP_KNN_CASE(16)
#undef THIP_KNN_CASE
  }
}
void launch_feat_knn_mutual_batch(hipStream_t s, const FeatSearchDesc* d_search, int n_pairs, int64_t max_entries,
                                  int k, const int32_t* d_idx, uint8_t* d_keep) {
  if (n_pairs <= 0 || max_entries <= 0) return;
  for (int p0 = 0; p0 < n_pairs; p0 += 65535)
    hipLaunchKernelGGL(feat_knn_mutual_batch_kernel, dim3((unsigned)((max_entries + 255) / 256),
                                                          std::min(65535, n_pairs - p0)),
                       dim3(256), 0, s, d_search, p0, k, d_idx, d_keep);
}

int64_t feat_tuple_blocks(int64_t ncorr) {
  const int64_t trials = 100 * ncorr;
  return std::max<int64_t>(1, std::min<int64_t>((trials + 255) / 256, kTupleMaxBlocks));
}
void launch_feat_tuple_batch(hipStream_t s, const FeatTupleDesc* d_desc, const int32_t* d_blk_problem, int blk_base,
                             int n_blk, const float* d_pts, const int32_t* d_pairs, uint8_t* d_keep) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(feat_tuple_batch_kernel, dim3(n_blk), dim3(256), 0, s, d_desc, d_blk_problem, blk_base, d_pts,
                     reinterpret_cast<const int2*>(d_pairs), d_keep);
}

}  // namespace thip
