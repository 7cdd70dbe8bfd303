// icp_cov_device.h -- the device functions that covariance estimation (kernels_icp.hip), normal estimation (both
// kernel files) and self k-NN (kernels_outlier.hip) share: the per-lane sorted neighbour list in LDS, the ordered
// covariance sums, the FP64 cyclic Jacobi with the choice of the normal, and the store of a normal with its
// orientation.  The arithmetic is the covariance contract's and the normals contract's (include/teaser_hip.h); every
// function is forced inline and indexes its small arrays with compile-time constants only, so everything stays in VGPRs.
#pragma once

#include <math.h>

#include "icp_internal.h"

namespace thip {

// Inserts (d2, j) into the lane's list (ascending (d2, j), at most cap <= CAP entries, m of them in use).  A repeated
// (d2, j) is recognised at its place in the list (or is beyond a full list's last entry, like the first time).
template <int CAP>
__device__ __forceinline__ void icp_knn_insert(double (*ld)[kIcpCovBlock], int32_t (*lj)[kIcpCovBlock], int lane,
                                               int cap, int& m, double d2, int32_t j) {
  int pos = m;  // the number of kept entries below (d2, j)
  while (pos > 0) {
    const double pd = ld[pos - 1][lane];
    if (!(d2 < pd || (d2 == pd && j < lj[pos - 1][lane]))) break;
    --pos;
  }
  if (pos > 0 && ld[pos - 1][lane] == d2 && lj[pos - 1][lane] == j) return;  // seen before
  if (pos == cap) return;                                                    // not among the cap best
  if (m < cap) ++m;
  for (int t = m - 1; t > pos; --t) {  // t <= cap - 1 < CAP
    ld[t][lane] = ld[t - 1][lane];
    lj[t][lane] = lj[t - 1][lane];
  }
  ld[pos][lane] = d2;
  lj[pos][lane] = j;
}

// Hybrid search: the cap smallest (d2, j) with d2 < r2 among the buckets of the 27 cells around x's cell.  A bucket
// reached through two neighbour cells repeats its candidates; icp_knn_insert drops the repeats.  Returns m.
template <int CAP>
__device__ __forceinline__ int icp_hybrid_list(double (*ld)[kIcpCovBlock], int32_t (*lj)[kIcpCovBlock], int lane,
                                               int cap, const IcpDesc& d, const double (&x)[3],
                                               const double* __restrict__ qs, const int32_t* __restrict__ qj,
                                               const int32_t* __restrict__ bstart) {
  const int64_t c0 = icp_cell(x[0], d.origin[0], d.inv_h), c1 = icp_cell(x[1], d.origin[1], d.inv_h),
                c2 = icp_cell(x[2], d.origin[2], d.inv_h);
  const double r2 = d.r2;
  int m = 0;
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int64_t b = d.b_off + icp_bucket(c0 + dx, c1 + dy, c2 + dz, d.tb_mask);
        const int32_t k1 = bstart[b + 1];
        for (int32_t k = bstart[b]; k < k1; ++k) {
          const double e0 = x[0] - qs[3 * (int64_t)k], e1 = x[1] - qs[3 * (int64_t)k + 1],
                       e2 = x[2] - qs[3 * (int64_t)k + 2];
          const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
          if (!(d2 < r2)) continue;
          icp_knn_insert<CAP>(ld, lj, lane, cap, m, d2, qj[k]);
        }
      }
  return m;
}

// One neighbour y of x into S1 = sum o and S2 = sum o o^T (upper triangle by rows), o = y - x.
__device__ __forceinline__ void icp_cov_add(double (&s1)[3], double (&s2)[6], const double* __restrict__ yp,
                                            const double (&x)[3]) {
  const double o0 = yp[0] - x[0], o1 = yp[1] - x[1], o2 = yp[2] - x[2];
  s1[0] += o0;
  s1[1] += o1;
  s1[2] += o2;
  s2[0] += o0 * o0;
  s2[1] += o0 * o1;
  s2[2] += o0 * o2;
  s2[3] += o1 * o1;
  s2[4] += o1 * o2;
  s2[5] += o2 * o2;
}

// cov = (S2 - S1 S1^T / m) / (m - 1), upper triangle {00, 01, 02, 11, 12, 22}
__device__ __forceinline__ void icp_cov_finish(const double (&s1)[3], const double (&s2)[6], int m, double (&a)[6]) {
  const double dm = (double)m, dm1 = (double)(m - 1);
  a[0] = (s2[0] - (s1[0] * s1[0]) / dm) / dm1;
  a[1] = (s2[1] - (s1[0] * s1[1]) / dm) / dm1;
  a[2] = (s2[2] - (s1[0] * s1[2]) / dm) / dm1;
  a[3] = (s2[3] - (s1[1] * s1[1]) / dm) / dm1;
  a[4] = (s2[4] - (s1[1] * s1[2]) / dm) / dm1;
  a[5] = (s2[5] - (s1[2] * s1[2]) / dm) / dm1;
}

// The sample covariance of the lane's finished list (m >= 3 entries), consumed in ascending (d2, j).
__device__ __forceinline__ void icp_list_cov(const int32_t (*lj)[kIcpCovBlock], int lane, int m,
                                             const double* __restrict__ cloud /* first point of the cloud */,
                                             const double (&x)[3], double (&a)[6]) {
  double s1[3] = {0.0, 0.0, 0.0}, s2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < m; ++k) icp_cov_add(s1, s2, cloud + 3 * (int64_t)lj[k][lane], x);
  icp_cov_finish(s1, s2, m, a);
}

// One Jacobi rotation of the symmetric 3 x 3 a = {a00, a01, a02, a11, a12, a22} in the (P, Q) plane, O the third
// index; V accumulates the rotations (columns = eigenvectors).  Indices are compile-time: everything stays in VGPRs.
__device__ __forceinline__ constexpr int icp_sym(int i, int j) {
  return i <= j ? (i == 0 ? j : i + j + 1) : (j == 0 ? i : i + j + 1);
}

template <int P, int Q, int O>
__device__ __forceinline__ bool icp_jacobi_rotate(double (&a)[6], double (&V)[9]) {
  constexpr int PQ = icp_sym(P, Q), PP = icp_sym(P, P), QQ = icp_sym(Q, Q), OP = icp_sym(O, P), OQ = icp_sym(O, Q);
  const double apq = a[PQ], app = a[PP], aqq = a[QQ];
  if (apq == 0.0 || fabs(apq) <= 1e-17 * (fabs(app) + fabs(aqq))) return false;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
  const double c = 1.0 / sqrt(1.0 + t * t), sn = t * c;
  a[PP] = app - t * apq;
  a[QQ] = aqq + t * apq;
  a[PQ] = 0.0;
  const double aop = a[OP], aoq = a[OQ];
  a[OP] = c * aop - sn * aoq;
  a[OQ] = sn * aop + c * aoq;
  const double v0p = V[P], v0q = V[Q], v1p = V[3 + P], v1q = V[3 + Q], v2p = V[6 + P], v2q = V[6 + Q];
  V[P] = c * v0p - sn * v0q;
  V[Q] = sn * v0p + c * v0q;
  V[3 + P] = c * v1p - sn * v1q;
  V[3 + Q] = sn * v1p + c * v1q;
  V[6 + P] = c * v2p - sn * v2q;
  V[6 + Q] = sn * v2p + c * v2q;
  return true;
}

// The cyclic Jacobi of the contract on a (its diagonal a[0], a[3], a[5] holds the eigenvalues afterwards) and the
// unit normal: the column of the smallest diagonal entry, the first one on a tie.
__device__ __forceinline__ void icp_cov_normal(double (&a)[6], double (&nrm)[3]) {
  double V[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  for (int sweep = 0; sweep < 16; ++sweep) {
    bool rotated = icp_jacobi_rotate<0, 1, 2>(a, V);
    rotated |= icp_jacobi_rotate<0, 2, 1>(a, V);
    rotated |= icp_jacobi_rotate<1, 2, 0>(a, V);
    if (!rotated) break;
  }
  // (selected value by value: a selected column index would turn V into a scratch array)
  const bool k1 = a[3] < a[0];
  const double lam = k1 ? a[3] : a[0];
  const bool k2 = a[5] < lam;
  nrm[0] = k2 ? V[2] : (k1 ? V[1] : V[0]);
  nrm[1] = k2 ? V[5] : (k1 ? V[4] : V[3]);
  nrm[2] = k2 ? V[8] : (k1 ? V[7] : V[6]);
  const double len = sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]);
  nrm[0] = nrm[0] / len;
  nrm[1] = nrm[1] / len;
  nrm[2] = nrm[2] / len;
}

// What a normal-estimation kernel writes to (kernel argument, by value).
struct IcpNormalOut {
  const IcpNormalDesc* nd;  // one per cloud
  double* nrm;              // 3 doubles per row, rows at IcpNormalDesc::nrm_off
  double* cov;              // 9 doubles per row at cov_off (clouds with cov_off >= 0)
  double* eig;              // 3 doubles per row at eig_off (clouds with eig_off >= 0)
};

// Point i (coordinates x) of a cloud with m neighbours, `a` the raw covariance of icp_cov_finish (read when m >= 3):
// Jacobi, the normal, its orientation, and the stores of the normal and of the optional covariance / eigenvalues.
__device__ __forceinline__ void icp_normal_store(const IcpNormalOut& out, const IcpNormalDesc& nd, int64_t i,
                                                 const double (&x)[3], int m, double (&a)[6]) {
  double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double e0 = 0.0, e1 = 0.0, e2 = 0.0;
  double nrm[3] = {0.0, 0.0, 0.0};
  const double r0 = nd.ref[0], r1 = nd.ref[1], r2 = nd.ref[2];
  if (m >= 3) {
    c[0] = a[0], c[1] = a[1], c[2] = a[2], c[3] = a[3], c[4] = a[4], c[5] = a[5];
    icp_cov_normal(a, nrm);
    e0 = a[0], e1 = a[3], e2 = a[5];  // ascending by three exchanges
    if (e1 < e0) { const double t = e0; e0 = e1; e1 = t; }
    if (e2 < e1) { const double t = e1; e1 = e2; e2 = t; }
    if (e1 < e0) { const double t = e0; e0 = e1; e1 = t; }
    double dot = 0.0;
    if (nd.orient == 1) dot = (nrm[0] * (r0 - x[0]) + nrm[1] * (r1 - x[1])) + nrm[2] * (r2 - x[2]);
    if (nd.orient == 2) dot = (nrm[0] * r0 + nrm[1] * r1) + nrm[2] * r2;
    if (dot < 0.0) {
      nrm[0] = -nrm[0];
      nrm[1] = -nrm[1];
      nrm[2] = -nrm[2];
    }
  } else if (nd.orient == 1) {  // the fill-ins of Open3D's orient_normals_* for a zero normal
    const double v0 = r0 - x[0], v1 = r1 - x[1], v2 = r2 - x[2];
    const double len = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    nrm[0] = len == 0.0 ? 0.0 : v0 / len;
    nrm[1] = len == 0.0 ? 0.0 : v1 / len;
    nrm[2] = len == 0.0 ? 1.0 : v2 / len;
  } else if (nd.orient == 2) {
    nrm[0] = r0, nrm[1] = r1, nrm[2] = r2;
  } else {
    nrm[2] = 1.0;
  }
  double* o = out.nrm + 3 * (nd.nrm_off + i);
  o[0] = nrm[0];
  o[1] = nrm[1];
  o[2] = nrm[2];
  if (nd.cov_off >= 0) {
    double* w = out.cov + 9 * (nd.cov_off + i);
    w[0] = c[0], w[1] = c[1], w[2] = c[2];
    w[3] = c[1], w[4] = c[3], w[5] = c[4];
    w[6] = c[2], w[7] = c[4], w[8] = c[5];
  }
  if (nd.eig_off >= 0) {
    double* w = out.eig + 3 * (nd.eig_off + i);
    w[0] = e0, w[1] = e1, w[2] = e2;
  }
}

}  // namespace thip
