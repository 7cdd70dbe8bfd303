// kernels_icp_color.hip -- the colour gradients of Colored ICP (include/teaser_hip.h, "ICP refinement: Colored ICP";
// Park, Zhou, Koltun, "Colored Point Cloud Registration Revisited", ICCV 2017) for gfx950.
//
// The shape of icp_normals_kernel: the ICP grid built over the cloud itself with the gradient radius, one point per
// lane, the gradient_max_nn smallest (d2, j) in the per-lane sorted list in LDS (icp_hybrid_list).  Then, by that lane,
// the sums over slots 1 .. m - 1 in list order -- the neighbour's point and intensity gathered by its original index --
// the orthogonality row, the 3 x 3 LDL^T and the store.  Every sum has a fixed order, so a cloud gives the same bits
// alone, in any batch and run after run.  The correspondence kernel that consumes the gradients: icp_corr_kernel<3>
// (kernels_icp.hip).
#include <math.h>

#include "icp_cov_device.h"
#include "icp_internal.h"

namespace thip {

// G d = h for the symmetric 3 x 3 G = {00, 01, 02, 11, 12, 22} by LDL^T without pivoting (the recurrences of
// icp_plane_step); d = 0 when a pivot is not finite or not > 0, or when d is not finite.
__device__ __forceinline__ void icp_color_solve3(const double (&G)[6], const double (&h)[3], double (&d)[3]) {
  d[0] = d[1] = d[2] = 0.0;
  const double p0 = G[0];
  if (!isfinite(p0) || !(p0 > 0.0)) return;
  const double l10 = G[1] / p0, l20 = G[2] / p0;
  const double p1 = G[3] - l10 * l10 * p0;
  if (!isfinite(p1) || !(p1 > 0.0)) return;
  const double l21 = (G[4] - l20 * l10 * p0) / p1;
  double p2 = G[5] - l20 * l20 * p0;
  p2 -= l21 * l21 * p1;
  if (!isfinite(p2) || !(p2 > 0.0)) return;
  double y0 = h[0];
  double y1 = h[1] - l10 * y0;
  double y2 = h[2] - l20 * y0;
  y2 -= l21 * y1;
  y0 = y0 / p0;
  y1 = y1 / p1;
  y2 = y2 / p2;
  const double x2 = y2;
  const double x1 = y1 - l21 * x2;
  double x0 = y0 - l10 * x1;
  x0 -= l20 * x2;
  if (!isfinite(x0) || !isfinite(x1) || !isfinite(x2)) return;
  d[0] = x0;
  d[1] = x1;
  d[2] = x2;
}


// rec: 4 doubles per point -- the gradient (written here), then the intensity (read here, of the point and of its
// neighbours); no lane writes what another reads.
template <int CAP>
__global__ __launch_bounds__(kIcpCovBlock) void icp_color_gradient_kernel(const IcpDesc* __restrict__ descs,
                                                                         const IcpGradDesc* __restrict__ gds,
                                                                         const int32_t* __restrict__ blk_prob,
                                                                         const double* __restrict__ q,
                                                                         const double* __restrict__ qs,
                                                                         const int32_t* __restrict__ qj,
                                                                         const int32_t* __restrict__ bstart,
                                                                         const double* __restrict__ normals,
                                                                         double* rec) {
  __shared__ double ld[CAP][kIcpCovBlock];   // slot-major: lane l owns ld[.][l]
  __shared__ int32_t lj[CAP][kIcpCovBlock];
  const int p = blk_prob[blockIdx.x];
  const IcpDesc& d = descs[p];
  const int lane = threadIdx.x;
  const int64_t i = (int64_t)((int)blockIdx.x - d.blk_off) * kIcpCovBlock + lane;
  if (i >= d.n_t) return;
  const int cap = gds[p].max_nn < CAP ? gds[p].max_nn : CAP;  // <= CAP: every list index stays inside
  const double* xp = q + 3 * (d.t_off + i);
  const double x[3] = {xp[0], xp[1], xp[2]};
  const int m = icp_hybrid_list<CAP>(ld, lj, lane, cap, d, x, qs, qj, bstart);
  double g[3] = {0.0, 0.0, 0.0};
  if (m >= 4) {
    const double* np = normals + 3 * (d.t_off + i);
    const double n[3] = {np[0], np[1], np[2]};
    const double ii = rec[4 * (d.t_off + i) + 3];
    double G[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, h[3] = {0.0, 0.0, 0.0};
    for (int k = 1; k < m; ++k) {  // slot 0 is skipped, whichever point it is
      const int64_t j = d.t_off + lj[k][lane];
      const double* yp = q + 3 * j;
      const double o0 = yp[0] - x[0], o1 = yp[1] - x[1], o2 = yp[2] - x[2];
      const double s = (o0 * n[0] + o1 * n[1]) + o2 * n[2];
      const double a0 = o0 - s * n[0], a1 = o1 - s * n[1], a2 = o2 - s * n[2];
      const double b = rec[4 * j + 3] - ii;
      G[0] += a0 * a0;
      G[1] += a0 * a1;
      G[2] += a0 * a2;
      G[3] += a1 * a1;
      G[4] += a1 * a2;
      G[5] += a2 * a2;
      h[0] += a0 * b;
      h[1] += a1 * b;
      h[2] += a2 * b;
    }
    const double w = (double)(m - 1);
    const double w0 = w * n[0], w1 = w * n[1], w2 = w * n[2];
    G[0] += w0 * w0;
    G[1] += w0 * w1;
    G[2] += w0 * w2;
    G[3] += w1 * w1;
    G[4] += w1 * w2;
    G[5] += w2 * w2;
    icp_color_solve3(G, h, g);
  }
  double* o = rec + 4 * (d.t_off + i);
  o[0] = g[0];
  o[1] = g[1];
  o[2] = g[2];
}

void launch_icp_color_gradients(hipStream_t s, const IcpDesc* d_desc, const IcpGradDesc* d_gd, const int32_t* d_blk_prob,
                                int n_blk, int max_nn, const double* d_q, const double* d_qs, const int32_t* d_qj,
                                const int32_t* d_bstart, const double* d_normals, double* d_rec) {
  if (n_blk <= 0) return;
  if (max_nn <= kIcpCovSmallNN)  // the capacity only bounds the list: it never changes a result
    hipLaunchKernelGGL(icp_color_gradient_kernel<kIcpCovSmallNN>, dim3(n_blk), dim3(kIcpCovBlock), 0, s, d_desc, d_gd,
                       d_blk_prob, d_q, d_qs, d_qj, d_bstart, d_normals, d_rec);
  else
    hipLaunchKernelGGL(icp_color_gradient_kernel<kIcpCovMaxNN>, dim3(n_blk), dim3(kIcpCovBlock), 0, s, d_desc, d_gd,
                       d_blk_prob, d_q, d_qs, d_qj, d_bstart, d_normals, d_rec);
}

}  // namespace thip
