// Host-only check of the two entries of csrc/icp.hip that no other host-only program runs (tests/test_icp_host.py):
// teaser_hip_icp_covariances_batch and teaser_hip_icp_batch_cov, compiled by g++ against the HIP stand-in header
// (tests/hip_stub), built with -fsanitize=address,undefined as a stand-alone program.  The launchers of the covariance
// and the iteration kernels are stand-ins that walk the block map as the kernels do and read and write every row the
// kernels would, with values derived from (problem, point): a buffer that is sized, packed or unpacked at a wrong offset
// is an AddressSanitizer report or a wrong value here.
//   icp_host_driver    exit code 0: every expectation met
// TEST INFRASTRUCTURE ONLY.
#define ICP_HOST_PRELUDE_OWN_ICP_LAUNCHERS
#include "icp_host_prelude.h"
#include "../teaser-plusplus_amd/csrc/icp.hip"

// coordinate c of point i of cloud p: distinct over everything a call packs
static double coord(int p, int i, int c) { return 1000.0 * p + i + 0.25 * c; }

static struct {
  int calls, n_blk, batch, mode, bad;
} g_it;

namespace thip {

// point i of cloud p gets the nine doubles coord(p, i, 0 .. 8) after a look at its own uploaded coordinates
void launch_icp_covariances(hipStream_t, const IcpDesc* desc, const IcpCovDesc* cov, const int32_t* blk_prob, int n_blk,
                            int max_nn, const double* q, const double*, const int32_t*, const int32_t*, double* out) {
  for (int blk = 0; blk < n_blk; ++blk) {
    const int p = blk_prob[blk];
    const IcpDesc& d = desc[p];
    for (int lane = 0; lane < kIcpCovBlock; ++lane) {
      const int64_t i = (int64_t)(blk - d.blk_off) * kIcpCovBlock + lane;
      if (i >= d.n_t) continue;
      expect(cov[p].max_nn <= max_nn && q[3 * (d.t_off + i)] == coord(p, (int)i, 0), "covariances: uploaded point", p);
      for (int c = 0; c < 9; ++c) out[9 * (d.t_off + i) + c] = coord(p, (int)i, c);
    }
  }
}

// One correspondence pass: every source point of every block looks at its own uploaded coordinates and, by method, at
// the last target's normal or covariance and its own covariance, and is matched with target i mod n_t; every block
// writes its partial sums.  What the launch was handed is recorded.
void launch_icp_iteration(hipStream_t, const IcpDesc* desc, IcpState* state, const int32_t* blk_prob, int n_blk,
                          int batch, double* x, const double* qs, const int32_t* qj, const int32_t* bstart,
                          const double* normals, const double* cov_s, const double* cov_t, int mode, int32_t* match,
                          double* partials) {
  ++g_it.calls;
  g_it.n_blk = n_blk, g_it.batch = batch, g_it.mode = mode;
  const int sums = mode ? kIcpPlaneSums : kIcpSums;
  for (int blk = 0; blk < n_blk; ++blk) {
    const int p = blk_prob[blk];
    const IcpDesc& d = desc[p];
    for (int k = 0; k < sums; ++k) partials[(int64_t)sums * blk + k] = 0.0;
    for (int lane = 0; lane < kIcpBlock; ++lane) {
      const int64_t i = (int64_t)(blk - d.blk_off) * kIcpBlock + lane;
      if (i >= d.n_s) continue;
      g_it.bad += x[3 * (d.s_off + i)] != coord(p, (int)i, 0);
      const int64_t last = d.t_off + d.n_t - 1;
      if (d.n_t > 0) {
        g_it.bad += qj[last] < 0 || qj[last] >= d.n_t || !std::isfinite(qs[3 * last + 2]);
        g_it.bad += bstart[d.b_off + d.tb_mask + 1] != (int32_t)(d.t_off + d.n_t);
        if (d.method == kIcpMethodPlane) g_it.bad += normals[3 * last + 2] != 0.5 + p;
        if (d.method == kIcpMethodGicp)
          g_it.bad += cov_t[6 * last + 5] != 7.0 + p || cov_s[6 * (d.s_off + i) + 5] != 9.0 + p;
      }
      match[d.s_off + i] = d.n_t > 0 ? (int32_t)(i % d.n_t) : -1;
    }
    state[p].count = 100 * p + d.n_s;
  }
}

}  // namespace thip

int main() {
  teaser_hip_icp* h = nullptr;
  if (teaser_hip_icp_create(0, &h) != TEASER_HIP_OK) return 2;
  auto cloud = [](int p, int n) {
    std::vector<double> q(3 * (size_t)n);
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < 3; ++c) q[3 * (size_t)i + c] = coord(p, i, c);
    return q;
  };

  // ---- covariance estimation: the block edges of kIcpCovBlock = 64 and of the 256-point target blocks ----
  {
    const int32_t n[4] = {0, 1, 65, 257}, max_nn[4] = {30, 3, 30, 100};
    const double radius[4] = {1.0, 2.0, 1.5, 3.0};
    std::vector<std::vector<double>> pts, out;
    for (int b = 0; b < 4; ++b) pts.push_back(cloud(b, n[b])), out.emplace_back(9 * (size_t)n[b], -1.0);
    const double* pp[4] = {nullptr, pts[1].data(), pts[2].data(), pts[3].data()};
    double* po[4] = {nullptr, out[1].data(), out[2].data(), out[3].data()};
    for (int round = 0; round < 2; ++round) {  // on fresh buffers, then on grown ones
      expect(teaser_hip_icp_covariances_batch(h, 4, pp, n, radius, max_nn, nullptr, po) == TEASER_HIP_OK,
             teaser_hip_icp_last_error(h), 0);
      for (int b = 0; b < 4; ++b)
        for (int i = 0; i < n[b]; ++i)
          for (int c = 0; c < 9; ++c)
            expect(out[(size_t)b][9 * (size_t)i + c] == coord(b, i, c), "covariances: a row of out is not its own", b);
    }
  }

  // ---- the iterations: point-to-point, point-to-plane with given normals, Generalized ICP with given covariances ----
  {
    const int32_t n_src[3] = {1, 257, 256}, n_dst[3] = {65, 64, 257};
    std::vector<std::vector<double>> src, dst, cs(3), ct(3);
    for (int b = 0; b < 3; ++b) src.push_back(cloud(b, n_src[b])), dst.push_back(cloud(b + 3, n_dst[b]));
    std::vector<double> normals(3 * (size_t)n_dst[1], 0.5 + 1);
    cs[2].assign(9 * (size_t)n_src[2], 9.0 + 2), ct[2].assign(9 * (size_t)n_dst[2], 7.0 + 2);
    const double* ps[3] = {src[0].data(), src[1].data(), src[2].data()};
    const double* pd[3] = {dst[0].data(), dst[1].data(), dst[2].data()};
    const double* pn[3] = {nullptr, normals.data(), nullptr};
    const double* pcs[3] = {nullptr, nullptr, cs[2].data()};
    const double* pct[3] = {nullptr, nullptr, ct[2].data()};
    teaser_icp_params_c prm[3];
    teaser_icp_estimation_c est[3];
    for (int b = 0; b < 3; ++b) {
      teaser_hip_icp_params_default(&prm[b]);
      prm[b].max_correspondence_distance = 0.5 + b;
      prm[b].max_iteration = 1;
      teaser_hip_icp_estimation_default(&est[b]);
      est[b].method = b;
    }
    teaser_icp_result_c out[3];
    std::vector<std::vector<int32_t>> corr;
    for (int b = 0; b < 3; ++b) corr.emplace_back(2 * (size_t)n_src[b], -7);
    int32_t* pc[3] = {corr[0].data(), corr[1].data(), corr[2].data()};
    int want_blk = 0;
    for (int b = 0; b < 3; ++b) want_blk += (n_src[b] + kIcpBlock - 1) / kIcpBlock;
    for (int with_corr = 0; with_corr < 2; ++with_corr) {
      g_it = {};
      expect(teaser_hip_icp_batch_cov(h, 3, ps, n_src, pd, n_dst, nullptr, prm, out, with_corr ? pc : nullptr, pn, est,
                                      pcs, pct) == TEASER_HIP_OK,
             teaser_hip_icp_last_error(h), 1);
      expect(g_it.calls == 2, "iterations: the first pass and one iteration", 1);
      expect(g_it.n_blk == want_blk && g_it.batch == 3, "iterations: n_blk is the sum of ceil(n_src / kIcpBlock)", 1);
      expect(g_it.mode == 2, "iterations: the mode of a batch with a Generalized-ICP problem", 1);
      expect(g_it.bad == 0, "iterations: a launch saw a row that is not its own", 1);
      for (int b = 0; b < 3; ++b) {
        expect(out[b].n_correspondences == 100 * b + n_src[b], "iterations: the state of another problem", b);
        for (int i = 0; with_corr && i < n_src[b]; ++i)
          expect(corr[(size_t)b][2 * (size_t)i] == i && corr[(size_t)b][2 * (size_t)i + 1] == i % n_dst[b],
                 "iterations: a correspondence of another point", b);
      }
    }
  }
  teaser_hip_icp_destroy(h);
  std::printf("mismatches %d\n", g_bad);
  return g_bad ? 1 : 0;
}
