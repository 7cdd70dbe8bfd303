// Host-only check of Colored ICP's host side (tests/test_icp_colored_host.py): csrc/icp.hip and csrc/icp_color.hip
// compiled by g++ against the HIP stand-in header (tests/hip_stub), with the SOURCE of the colour-gradient kernel
// (csrc/kernels_icp_color.hip: lane-independent, so the stand-in header runs it one lane at a time), built with
// -fsanitize=address,undefined as a stand-alone program.  "Device" buffers are host allocations of exactly the size the
// host code asked for, so a plan, a record layout or an upload that is sized or addressed wrongly is an AddressSanitizer
// report.  The launcher of the mode-3 iteration is a stand-in that walks the block map as the kernel does and reads
// every row the kernel would: the per-problem records, the source intensities, the normals, and the {gradient,
// intensity} records -- given gradients as given, estimated ones equal, bit for bit, to what
// teaser_hip_icp_color_gradients_batch returns for the same cloud.
//   icp_colored_host_driver    exit code 0: every expectation met
// TEST INFRASTRUCTURE ONLY.
#include "icp_host_prelude.h"
#include "../teaser-plusplus_amd/csrc/kernels_icp_color.hip"
#include "../teaser-plusplus_amd/csrc/icp.hip"
#include "../teaser-plusplus_amd/csrc/icp_color.hip"

// the clouds: an exact plane z = 0 on a lattice (spacing 0.1, 16 points per row), intensity linear in x and y
static double coord(int p, int i, int c) { return c == 0 ? 0.1 * (i % 16) + p : c == 1 ? 0.1 * (i / 16) : 0.0; }
static double colour(int p, int i, int c) { return 0.25 * coord(p, i, 0) - 0.5 * coord(p, i, 1) + 0.125 * c + 0.0625 * p; }
static double inten(int p, int i) { return ((colour(p, i, 0) + colour(p, i, 1)) + colour(p, i, 2)) / 3.0; }

struct Want {
  int method = 0;
  double lambda = 0;
  const double* normals = nullptr;
  const double* grad = nullptr;  // what the records must hold: given, or estimated by the gradients call
  int src_cloud = 0, dst_cloud = 0;
};
static std::vector<Want> g_want;
static struct {
  int calls, n_blk, batch, bad;
} g_it;

namespace thip {

void launch_icp_iteration_color(hipStream_t, const IcpDesc* desc, IcpState* state, const int32_t* blk_prob, int n_blk,
                                int batch, double* x, const double* qs, const int32_t* qj, const int32_t* bstart,
                                const double* normals, const double*, const double*, int32_t* match, double* partials,
                                const IcpColorArgs& col) {
  ++g_it.calls;
  g_it.n_blk = n_blk, g_it.batch = batch;
  for (int blk = 0; blk < n_blk; ++blk) {
    const int p = blk_prob[blk];
    const IcpDesc& d = desc[p];
    const Want& w = g_want[(size_t)p];
    for (int k = 0; k < kIcpPlaneSums; ++k) partials[(int64_t)kIcpPlaneSums * blk + k] = 0.0;
    g_it.bad += d.method != w.method;
    if (d.method == kIcpMethodColor)
      g_it.bad += col.cd[p].sg != sqrt(w.lambda) || col.cd[p].sp != sqrt(1.0 - w.lambda);
    for (int lane = 0; lane < kIcpBlock; ++lane) {
      const int64_t i = (int64_t)(blk - d.blk_off) * kIcpBlock + lane;
      if (i >= d.n_s) continue;
      g_it.bad += x[3 * (d.s_off + i)] != coord(w.src_cloud, (int)i, 0);
      if (d.method == kIcpMethodColor) g_it.bad += col.int_s[d.s_off + i] != inten(w.src_cloud, (int)i);
      match[d.s_off + i] = d.n_t > 0 ? (int32_t)(i % d.n_t) : -1;
    }
    if (d.n_t > 0) {
      const int64_t last = d.t_off + d.n_t - 1;
      g_it.bad += qj[last] < 0 || qj[last] >= d.n_t || !std::isfinite(qs[3 * last + 2]);
      g_it.bad += bstart[d.b_off + d.tb_mask + 1] != (int32_t)(d.t_off + d.n_t);
    }
    if (d.method == kIcpMethodColor || d.method == kIcpMethodPlane)
      for (int64_t j = 0; j < d.n_t; ++j)
        for (int c = 0; c < 3; ++c) g_it.bad += normals[3 * (d.t_off + j) + c] != w.normals[3 * j + c];
    if (d.method == kIcpMethodColor)
      for (int64_t j = 0; j < d.n_t; ++j) {
        const double* rec = col.rec_t + 4 * (d.t_off + j);
        g_it.bad += rec[3] != inten(w.dst_cloud, (int)j);
        g_it.bad += memcmp(rec, w.grad + 3 * j, 24) != 0;
      }
    state[p].count = 100 * p + d.n_s;
  }
}

}  // namespace thip

int main() {
  teaser_hip_icp* h = nullptr;
  if (teaser_hip_icp_create(0, &h) != TEASER_HIP_OK) return 2;
  auto fill = [](int p, int n, double (*f)(int, int, int)) {
    std::vector<double> q(3 * (size_t)n);
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < 3; ++c) q[3 * (size_t)i + c] = f(p, i, c);
    return q;
  };
  auto up = [](int, int, int c) { return c == 2 ? 1.0 : 0.0; };

  // ---- the gradients call: the block edges of kIcpCovBlock = 64 and of the 256-point target blocks ----
  const int32_t n[4] = {0, 65, 257, 130}, max_nn[4] = {30, 4, 33, 30};
  const double radius[4] = {1.0, 0.25, 0.35, 0.25};
  std::vector<std::vector<double>> pts, nrm, col, grad;
  for (int b = 0; b < 4; ++b) {
    pts.push_back(fill(b, n[b], coord)), nrm.push_back(fill(b, n[b], up)), col.push_back(fill(b, n[b], colour));
    grad.emplace_back(3 * (size_t)n[b], -1.0);
  }
  {
    const double* pp[4] = {nullptr, pts[1].data(), pts[2].data(), pts[3].data()};
    const double* pn[4] = {nullptr, nrm[1].data(), nrm[2].data(), nrm[3].data()};
    const double* pc[4] = {nullptr, col[1].data(), col[2].data(), col[3].data()};
    double* po[4] = {nullptr, grad[1].data(), grad[2].data(), grad[3].data()};
    for (int round = 0; round < 2; ++round) {  // on fresh buffers, then on grown ones
      expect(teaser_hip_icp_color_gradients_batch(h, 4, pp, n, pn, pc, radius, max_nn, po) == TEASER_HIP_OK,
             teaser_hip_icp_last_error(h), 0);
      for (int b = 1; b < 4; ++b)
        for (int i = 0; i < n[b]; ++i) {  // I = 0.25 x - 0.5 y + const on the plane z = 0: the gradient is (0.25, -0.5, 0)
          const double* g = &grad[(size_t)b][3 * (size_t)i];
          expect(std::fabs(g[0] - 0.25) < 1e-9 && std::fabs(g[1] + 0.5) < 1e-9 && std::fabs(g[2]) < 1e-9,
                 "gradients: not the tangential part of the linear intensity", b);
        }
    }
    std::vector<double> alone(3 * (size_t)n[2], -1.0);
    double* pa = alone.data();
    expect(teaser_hip_icp_color_gradients_batch(h, 1, &pp[2], &n[2], &pn[2], &pc[2], &radius[2], &max_nn[2], &pa) ==
               TEASER_HIP_OK && same(alone, grad[2]),
           "gradients: a cloud alone is not what it is in the batch", 2);
    const int32_t three = 3;
    expect(teaser_hip_icp_color_gradients_batch(h, 1, &pp[1], &n[1], &pn[1], &pc[1], &radius[1], &three, &po[1]) ==
               TEASER_HIP_ERR_BAD_ARG && std::string(teaser_hip_icp_last_error(h)).find("max_nn") != std::string::npos,
           "gradients: max_nn 3 is refused", 1);
  }

  // ---- the iterations: the four methods in one call; coloured problems with estimated and with given gradients ----
  {
    // problem b: source cloud b of n_src points, target = gradient cloud dst_cloud[b]
    const int nb = 6;
    const int32_t n_src[nb] = {1, 257, 256, 300, 70, 0}, dst_cloud[nb] = {1, 3, 1, 2, 3, 1};
    const int method[nb] = {0, 1, 2, 3, 3, 3};
    std::vector<std::vector<double>> src, scol, cs(nb), ct(nb);
    std::vector<double> given(3 * (size_t)n[3]);
    for (size_t k = 0; k < given.size(); ++k) given[k] = 0.5 + (double)k;
    const double *ps[nb], *pd[nb], *pn[nb], *pcs[nb], *pct[nb], *psc[nb], *pdc[nb], *pg[nb];
    int32_t n_dst[nb];
    teaser_icp_params_c prm[nb];
    teaser_icp_estimation_c est[nb];
    teaser_icp_color_c rec[nb];
    g_want.assign(nb, Want());
    for (int b = 0; b < nb; ++b) {
      const int t = dst_cloud[b];
      src.push_back(fill(b, n_src[b], coord)), scol.push_back(fill(b, n_src[b], colour));
      ps[b] = src[(size_t)b].data(), pd[b] = pts[(size_t)t].data(), n_dst[b] = n[t];
      pn[b] = method[b] == 1 || method[b] == 3 ? nrm[(size_t)t].data() : nullptr;
      pcs[b] = pct[b] = psc[b] = pdc[b] = pg[b] = nullptr;
      if (method[b] == 2) {
        cs[(size_t)b].assign(9 * (size_t)n_src[b], 1.0), ct[(size_t)b].assign(9 * (size_t)n_dst[b], 1.0);
        pcs[b] = cs[(size_t)b].data(), pct[b] = ct[(size_t)b].data();
      }
      if (method[b] == 3) psc[b] = scol[(size_t)b].data(), pdc[b] = col[(size_t)t].data();
      teaser_hip_icp_params_default(&prm[b]);
      prm[b].max_correspondence_distance = 0.5 * radius[t];  // the default gradient radius is then radius[t]
      prm[b].max_iteration = 1;
      teaser_hip_icp_estimation_default(&est[b]);
      est[b].method = method[b];
      teaser_hip_icp_color_default(&rec[b]);
      rec[b].lambda_geometric = 0.5 + 0.1 * b;
      rec[b].gradient_max_nn = max_nn[t];
      Want& w = g_want[(size_t)b];
      w.method = method[b], w.lambda = rec[b].lambda_geometric, w.normals = pn[b], w.src_cloud = b, w.dst_cloud = t;
      w.grad = grad[(size_t)t].data();
    }
    pg[4] = given.data(), g_want[4].grad = given.data();  // problem 4: its gradients are given
    rec[3].gradient_radius = radius[2];                   // problem 3: the radius given explicitly
    teaser_icp_result_c out[nb];
    std::vector<std::vector<int32_t>> corr;
    for (int b = 0; b < nb; ++b) corr.emplace_back(2 * (size_t)std::max(n_src[b], 1), -7);
    int32_t* pc[nb];
    for (int b = 0; b < nb; ++b) pc[b] = corr[(size_t)b].data();
    int want_blk = 0;
    for (int b = 0; b < nb; ++b) want_blk += (n_src[b] + kIcpBlock - 1) / kIcpBlock;
    for (int round = 0; round < 2; ++round) {
      g_it = {};
      expect(teaser_hip_icp_batch_color(h, nb, ps, n_src, pd, n_dst, nullptr, prm, out, round ? pc : nullptr, pn, est,
                                        pcs, pct, psc, pdc, pg, rec) == TEASER_HIP_OK,
             teaser_hip_icp_last_error(h), 1);
      expect(g_it.calls == 2, "iterations: the first pass and one iteration, through the mode-3 launcher", 1);
      expect(g_it.n_blk == want_blk && g_it.batch == nb, "iterations: n_blk is the sum of ceil(n_src / kIcpBlock)", 1);
      expect(g_it.bad == 0, "iterations: a launch saw a row that is not its own", 1);
      for (int b = 0; b < nb; ++b) {
        if (n_src[b] > 0) expect(out[b].n_correspondences == 100 * b + n_src[b], "iterations: another problem's state", b);
        for (int i = 0; round && i < n_src[b]; ++i)
          expect(corr[(size_t)b][2 * (size_t)i] == i && corr[(size_t)b][2 * (size_t)i + 1] == i % n_dst[b],
                 "iterations: a correspondence of another point", b);
      }
    }
    // without a coloured problem the call is teaser_hip_icp_batch_cov's: the mode-3 launcher is not reached
    g_it = {};
    expect(teaser_hip_icp_batch_color(h, 3, ps, n_src, pd, n_dst, nullptr, prm, out, nullptr, pn, est, pcs, pct, nullptr,
                                      nullptr, nullptr, nullptr) == TEASER_HIP_OK && g_it.calls == 0,
           "a call without a coloured problem reached the mode-3 launcher", 2);
    // refusals that never reach a launch
    expect(teaser_hip_icp_batch_cov(h, nb, ps, n_src, pd, n_dst, nullptr, prm, out, nullptr, pn, est, pcs, pct) ==
               TEASER_HIP_ERR_BAD_ARG && std::string(teaser_hip_icp_last_error(h)).find("method") != std::string::npos,
           "method 3 through _cov is refused", 3);
    psc[3] = nullptr;
    expect(teaser_hip_icp_batch_color(h, nb, ps, n_src, pd, n_dst, nullptr, prm, out, nullptr, pn, est, pcs, pct, psc,
                                      pdc, pg, rec) == TEASER_HIP_ERR_BAD_ARG &&
               std::string(teaser_hip_icp_last_error(h)).find("src_colors") != std::string::npos,
           "missing source colours are refused", 3);
  }
  teaser_hip_icp_destroy(h);
  std::printf("mismatches %d\n", g_bad);
  return g_bad ? 1 : 0;
}
