// icp_color_device.h -- what one Colored-ICP correspondence (include/teaser_hip.h, "ICP refinement: Colored ICP") adds
// to the 29-value partial of icp_corr_kernel<3>; included by kernels_icp.hip behind icp_kernel_weight.  Forced inline,
// its small arrays indexed with compile-time constants only, so everything stays in VGPRs.  No fused operations
// (-ffp-contract=off).
#pragma once

#include <math.h>

#include "icp_internal.h"

namespace thip {

// What one Colored-ICP correspondence adds to v[2..28].  pc, qc: the moved source point and its match, centred;
// n: the match's normal; rec: its colour gradient and intensity; is: the source intensity.
__device__ __forceinline__ void icp_color_terms(const double (&pc)[3], const double (&qc)[3], const double (&n)[3],
                                                const double* __restrict__ rec, double is, const IcpColorDesc& cd,
                                                int kernel, double kernel_k, double (&v)[kIcpPlaneSums]) {
  const double dg[3] = {rec[0], rec[1], rec[2]};
  const double it = rec[3];
  const double sg = cd.sg, sp = cd.sp;
  const double e0 = pc[0] - qc[0], e1 = pc[1] - qc[1], e2 = pc[2] - qc[2];
  const double s = (e0 * n[0] + e1 * n[1]) + e2 * n[2];
  double Jg[6], Ji[6];
  Jg[0] = sg * (pc[1] * n[2] - pc[2] * n[1]);
  Jg[1] = sg * (pc[2] * n[0] - pc[0] * n[2]);
  Jg[2] = sg * (pc[0] * n[1] - pc[1] * n[0]);
  Jg[3] = sg * n[0];
  Jg[4] = sg * n[1];
  Jg[5] = sg * n[2];
  const double rg = sg * s;
  const double wg = kernel == kIcpKernelL2 ? 1.0 : icp_kernel_weight(kernel, kernel_k, rg);
  const double u0 = e0 - s * n[0], u1 = e1 - s * n[1], u2 = e2 - s * n[2];
  const double isp = ((dg[0] * u0 + dg[1] * u1) + dg[2] * u2) + it;
  const double t = (dg[0] * n[0] + dg[1] * n[1]) + dg[2] * n[2];
  const double dm[3] = {t * n[0] - dg[0], t * n[1] - dg[1], t * n[2] - dg[2]};
  Ji[0] = sp * (pc[1] * dm[2] - pc[2] * dm[1]);
  Ji[1] = sp * (pc[2] * dm[0] - pc[0] * dm[2]);
  Ji[2] = sp * (pc[0] * dm[1] - pc[1] * dm[0]);
  Ji[3] = sp * dm[0];
  Ji[4] = sp * dm[1];
  Ji[5] = sp * dm[2];
  const double ri = sp * (is - isp);
  const double wi = kernel == kIcpKernelL2 ? 1.0 : icp_kernel_weight(kernel, kernel_k, ri);
  const double wrg = wg * rg, wri = wi * ri;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const double wjg = wg * Jg[r], wji = wi * Ji[r];
#pragma unroll
    for (int c = 0; c < 6; ++c)
      if (c >= r) v[2 + 6 * r - r * (r - 1) / 2 + (c - r)] = wjg * Jg[c] + wji * Ji[c];  // upper triangle by rows
  }
#pragma unroll
  for (int r = 0; r < 6; ++r) v[23 + r] = wrg * Jg[r] + wri * Ji[r];
}

}  // namespace thip
