// Host-only check of normal estimation (tests/test_normals_host.py): csrc/icp.hip, csrc/icp_outlier.hip and csrc/icp_normals.hip compiled by
// g++ against the HIP stand-in header, with the SOURCE of the lane-independent device code -- icp_cov_device.h and the
// ring kernel of csrc/kernels_outlier.hip with its covariance consumer -- run one lane at a time (tests/hip_stub runs a
// launch sequentially), built with -fsanitize=address,undefined.  "Device" buffers are host allocations of exactly the
// size the host code asked for, so a descriptor, an output layout or a worklist that is sized or addressed wrongly is an
// AddressSanitizer report; the results are compared bit for bit with tests/normals_reference.py, read from a text file.
// The hybrid kernel's ten-line shell lives in kernels_icp.hip, which does not compile for the host (wave reductions);
// it is restated below on the same device functions.  The scan kernel's wave merge CANNOT be emulated one lane at a
// time: no query of these cases reaches the worklist (asserted), and the scan launch finds it empty.
//   normals_host_driver CASES.txt    exit code 0: every case equal and every refusal refused
// TEST INFRASTRUCTURE ONLY.
#include "icp_host_prelude.h"
#include "../teaser-plusplus_amd/csrc/kernels_outlier.hip"
#include "../teaser-plusplus_amd/csrc/icp.hip"
#include "../teaser-plusplus_amd/csrc/icp_outlier.hip"
#include "../teaser-plusplus_amd/csrc/icp_normals.hip"

namespace thip {

// icp_normals_kernel of kernels_icp.hip, restated on the same device functions
template <int CAP>
void normals_kernel_shell(const IcpDesc* descs, const int32_t* blk_prob, const double* q, const double* qs,
                          const int32_t* qj, const int32_t* bstart, const IcpNormalOut out) {
  static double ld[CAP][kIcpCovBlock];
  static int32_t lj[CAP][kIcpCovBlock];
  const int p = blk_prob[blockIdx.x];
  const IcpDesc& d = descs[p];
  const IcpNormalDesc& nd = out.nd[p];
  const int lane = threadIdx.x;
  const int64_t i = (int64_t)((int)blockIdx.x - d.blk_off) * kIcpCovBlock + lane;
  if (i >= d.n_t) return;
  const int cap = nd.max_nn < CAP ? nd.max_nn : CAP;
  const double* xp = q + 3 * (d.t_off + i);
  const double x[3] = {xp[0], xp[1], xp[2]};
  const int m = icp_hybrid_list<CAP>(ld, lj, lane, cap, d, x, qs, qj, bstart);
  double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (m >= 3) icp_list_cov(lj, lane, m, q + 3 * d.t_off, x, a);
  icp_normal_store(out, nd, i, x, m, a);
}

void launch_icp_normals_hybrid(hipStream_t s, const IcpDesc* d_desc, const IcpNormalDesc* d_nd,
                               const int32_t* d_blk_prob, int n_blk, int max_nn, const double* d_q, const double* d_qs,
                               const int32_t* d_qj, const int32_t* d_bstart, double* d_nrm, double* d_cov,
                               double* d_eig) {
  if (n_blk <= 0) return;
  const IcpNormalOut out = {d_nd, d_nrm, d_cov, d_eig};
  if (max_nn <= kIcpCovSmallNN)
    hipLaunchKernelGGL(normals_kernel_shell<kIcpCovSmallNN>, dim3(n_blk), dim3(kIcpCovBlock), 0, s, d_desc, d_blk_prob,
                       d_q, d_qs, d_qj, d_bstart, out);
  else
    hipLaunchKernelGGL(normals_kernel_shell<kIcpCovMaxNN>, dim3(n_blk), dim3(kIcpCovBlock), 0, s, d_desc, d_blk_prob,
                       d_q, d_qs, d_qj, d_bstart, out);
}

}  // namespace thip

struct Case {
  int n = 0, search = 0, max_nn = 0, orient = 0;
  double radius = 0, ref[3] = {0, 0, 0};
  std::vector<double> pts, nrm, cov, eig;
};

static teaser_icp_normal_search_c record(const Case& c) {
  teaser_icp_normal_search_c r;
  memset(&r, 0, sizeof(r));
  r.search = c.search, r.max_nn = c.max_nn, r.radius = c.radius, r.orient = c.orient;
  for (int k = 0; k < 3; ++k) r.ref[k] = c.ref[k];
  return r;
}

// Worklist entries of the ring search (its own source, one lane at a time) on one cloud at ring cap 4.
static int worklist_entries(const std::vector<double>& q, int k) {
  const int n = (int)q.size() / 3;
  IcpDesc d{};
  IcpKnnDesc kd{};
  d.n_t = n, kd.k = k, kd.ring_cap = 4;
  bool rings_ok = true;
  kd.edge = knn_edge(q.data(), n, std::min(k, n), &rings_ok);
  d.r2 = kd.edge * kd.edge;
  set_grid(d, q.data(), kd.edge);
  std::vector<int32_t> bstart((size_t)d.tb_mask + 2, 0), qj((size_t)n), work(2 * (size_t)n), cnt(1, 0),
      idx((size_t)n * k), blk((size_t)(n + 63) / 64, 0);
  std::vector<double> qs(3 * (size_t)n), d2((size_t)n * k);
  launch_icp_index(nullptr, &d, nullptr, 0, 1, q.data(), nullptr, nullptr, bstart.data(), nullptr, qs.data(), qj.data());
  hipLaunchKernelGGL(icp_knn_ring_kernel<kIcpKnnMax>, dim3((n + 63) / 64), dim3(kIcpCovBlock), 0, nullptr, &d, &kd,
                     blk.data(), q.data(), qs.data(), qj.data(), bstart.data(), idx.data(), d2.data(), (double*)nullptr,
                     work.data(), cnt.data());
  return cnt[0];
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n_cases = 0;
  if (std::fscanf(f, "%d", &n_cases) != 1) return 2;
  std::vector<Case> cases((size_t)n_cases);
  for (Case& c : cases) {
    c.n = (int)read_number(f), c.search = (int)read_number(f), c.max_nn = (int)read_number(f);
    c.orient = (int)read_number(f), c.radius = read_number(f);
    for (int k = 0; k < 3; ++k) c.ref[k] = read_number(f);
    read_numbers(f, c.pts, 3 * (size_t)c.n);
    read_numbers(f, c.nrm, 3 * (size_t)c.n);
    read_numbers(f, c.cov, 9 * (size_t)c.n);
    read_numbers(f, c.eig, 3 * (size_t)c.n);
  }
  std::vector<double> planted;  // outlier_reference.planted_cloud(), after the cases
  int n_planted = 0;
  if (std::fscanf(f, "%d", &n_planted) != 1) return 2;
  read_numbers(f, planted, 3 * (size_t)n_planted);
  std::fclose(f);
  // what tests/test_gpu_normals.py expects of the planted cloud at ring cap 4: k = 10 reaches the worklist, k = 30 not
  const int fell10 = worklist_entries(planted, 10), fell30 = worklist_entries(planted, 30);
  std::printf("planted cloud: worklist entries %d at k = 10, %d at k = 30\n", fell10, fell30);
  expect(fell10 > 0 && fell10 < n_planted && fell30 == 0, "planted cloud: worklist entries", -3);

  teaser_hip_icp* h = nullptr;
  if (teaser_hip_icp_create(0, &h) != TEASER_HIP_OK) return 2;
  const int B = n_cases;
  for (int subset = 0; subset < 4; ++subset)  // which optional outputs are asked for: bit 0 covariances, bit 1 eigenvalues
    for (int pass = 0; pass < 2; ++pass) {    // pass 0: every case alone; pass 1: all of them in one batch
      if (pass == 0 && subset != 3) continue;
      for (int lo = 0; lo < B; lo += pass ? B : 1) {
        const int b = pass ? B : 1;
        std::vector<const double*> pp((size_t)b);
        std::vector<int32_t> n((size_t)b);
        std::vector<teaser_icp_normal_search_c> rec((size_t)b);
        std::vector<std::vector<double>> nrm((size_t)b), cov((size_t)b), eig((size_t)b);
        std::vector<double*> pn((size_t)b), pc((size_t)b), pe((size_t)b);
        for (int c = 0; c < b; ++c) {
          const Case& cs = cases[(size_t)(lo + c)];
          const size_t m = (size_t)cs.n;
          pp[c] = m ? cs.pts.data() : nullptr;
          n[c] = cs.n;
          rec[c] = record(cs);
          nrm[c].resize(3 * m), cov[c].resize(9 * m), eig[c].resize(3 * m);
          // in the batch every other cloud leaves out an optional output the call as a whole asks for
          const bool skip = pass && (c % 2 == 1);
          pn[c] = m ? nrm[c].data() : nullptr;
          pc[c] = m && (subset & 1) && !skip ? cov[c].data() : nullptr;
          pe[c] = m && (subset & 2) && !(pass && c % 3 == 1) ? eig[c].data() : nullptr;
        }
        expect(teaser_hip_icp_normals_batch(h, b, pp.data(), n.data(), rec.data(), pn.data(),
                                            (subset & 1) ? pc.data() : nullptr, (subset & 2) ? pe.data() : nullptr) == 0,
               teaser_hip_icp_last_error(h), lo);
        int64_t fell = -1;
        teaser_hip_icp_get_option(h, "knn_fallbacks", &fell);
        expect(fell == 0, "a query reached the worklist (the scan kernel is not emulated)", lo);
        for (int c = 0; c < b; ++c) {
          const Case& cs = cases[(size_t)(lo + c)];
          expect(same(nrm[c], cs.nrm), "normals", lo + c);
          if (pc[c]) expect(same(cov[c], cs.cov), "covariances", lo + c);
          if (pe[c]) expect(same(eig[c], cs.eig), "eigenvalues", lo + c);
        }
      }
    }

  // the self-estimating point-to-plane entry: estimated, given, empty, estimated; the iterations are stand-ins, the
  // rows of the packed normals buffer are what is checked
  if (B >= 3) {
    const Case &a = cases[0], &g = cases[1], &z = cases[2];
    const double* dst[5] = {a.pts.data(), g.pts.data(), nullptr, z.pts.data(), g.pts.data()};
    const int32_t n_dst[5] = {a.n, g.n, 0, z.n, g.n};
    const double one[3] = {0.5, 0.5, 0.5};
    const double* src[5] = {one, one, one, one, one};
    const int32_t n_src[5] = {1, 1, 1, 1, 1};
    std::vector<double> given(3 * (size_t)g.n, 0.25);
    const double* normals[5] = {nullptr, given.data(), nullptr, nullptr, nullptr};
    teaser_icp_params_c prm[5];
    teaser_icp_estimation_c est[5];
    for (int k = 0; k < 5; ++k) {
      teaser_hip_icp_params_default(&prm[k]);
      prm[k].max_correspondence_distance = 0.1;
      prm[k].max_iteration = 1;
      est[k].method = k == 4 ? 0 : 1, est[k].kernel = 0, est[k].kernel_k = 1.0;
    }
    teaser_icp_normal_search_c rec[5] = {record(a), record(a), record(a), record(z), record(a)};
    rec[1].search = 9;  // never read: the problem gives its normals
    rec[4].orient = 9;  // never read: point-to-point
    teaser_icp_result_c out[5];
    expect(teaser_hip_icp_batch_auto(h, 5, src, n_src, dst, n_dst, nullptr, prm, out, nullptr, normals, est, nullptr,
                                     nullptr, rec) == 0,
           teaser_hip_icp_last_error(h), -2);
    const double* dn = h->buf[B_NORMALS].as<double>();
    expect(memcmp(dn, a.nrm.data(), 24 * (size_t)a.n) == 0, "auto: estimated rows of problem 0", -2);
    expect(memcmp(dn + 3 * a.n, given.data(), 24 * (size_t)g.n) == 0, "auto: given rows of problem 1", -2);
    expect(memcmp(dn + 3 * (a.n + g.n), z.nrm.data(), 24 * (size_t)z.n) == 0, "auto: estimated rows of problem 3", -2);
    rec[0].max_nn = 0;  // "none given": the old refusal, by name
    const int32_t rc = teaser_hip_icp_batch_auto(h, 5, src, n_src, dst, n_dst, nullptr, prm, out, nullptr, normals, est,
                                                 nullptr, nullptr, rec);
    expect(rc == TEASER_HIP_ERR_BAD_ARG && std::string(teaser_hip_icp_last_error(h)).find("dst_normals") != std::string::npos,
           "auto: neither normals nor a record", -2);
    rec[0] = record(a);
    rec[3].max_nn = 2;
    expect(teaser_hip_icp_batch_auto(h, 5, src, n_src, dst, n_dst, nullptr, prm, out, nullptr, normals, est, nullptr,
                                     nullptr, rec) == TEASER_HIP_ERR_BAD_ARG &&
               std::string(teaser_hip_icp_last_error(h)).find("dst_normal_search: max_nn") != std::string::npos &&
               std::string(teaser_hip_icp_last_error(h)).find("problem 3") != std::string::npos,
           "auto: a bad record is refused by name", -2);
  }

  // refusals: BAD_ARG, the argument and the cloud named, and the handle still works
  {
    const Case& cs = cases[0];
    const double* pp[2] = {cs.pts.data(), cs.pts.data()};
    std::vector<double> bad = cs.pts;
    bad[4] = NAN;
    const double* pbad[2] = {cs.pts.data(), bad.data()};
    const int32_t n[2] = {cs.n, cs.n};
    std::vector<double> o0(3 * (size_t)cs.n), o1(3 * (size_t)cs.n);
    double* po[2] = {o0.data(), o1.data()};
    auto refused = [&](const double* const* pts, teaser_icp_normal_search_c r1, double* const* out, const char* w1) {
      teaser_icp_normal_search_c rec[2] = {record(cs), r1};
      const int32_t rc = teaser_hip_icp_normals_batch(h, 2, pts, n, rec, out, nullptr, nullptr);
      const std::string msg = teaser_hip_icp_last_error(h);
      expect(rc == TEASER_HIP_ERR_BAD_ARG && msg.find(w1) != std::string::npos &&
                 msg.find(out ? "problem 1" : "problem 0") != std::string::npos,
             (std::string("refusal: ") + w1 + " / " + msg).c_str(), -1);
    };
    auto with = [&](auto edit) {
      teaser_icp_normal_search_c r = record(cs);
      r.search = 0, r.radius = 0.3, r.orient = 1;
      edit(r);
      return r;
    };
    refused(pbad, record(cs), po, "points");
    refused(pp, with([](auto& r) { r.search = 2; }), po, "search");
    refused(pp, with([](auto& r) { r.search = -1; }), po, "search");
    refused(pp, with([](auto& r) { r.orient = 3; }), po, "orient");
    refused(pp, with([](auto& r) { r.reserved = 1; }), po, "reserved");
    refused(pp, with([](auto& r) { r.max_nn = 2; }), po, "max_nn");
    refused(pp, with([](auto& r) { r.max_nn = 101; }), po, "max_nn");
    refused(pp, with([](auto& r) { r.radius = 0.0; }), po, "radius");
    refused(pp, with([](auto& r) { r.radius = NAN; }), po, "radius");
    refused(pp, with([](auto& r) { r.radius = 1e200; }), po, "radius");
    refused(pp, with([](auto& r) { r.ref[1] = INFINITY; }), po, "ref");
    refused(pp, record(cs), nullptr, "normals_out");
    teaser_icp_normal_search_c fine[2] = {with([](auto& r) { r.search = 1, r.radius = NAN; }),
                                          with([](auto& r) { r.orient = 0, r.ref[0] = NAN; })};
    expect(teaser_hip_icp_normals_batch(h, 2, pp, n, fine, po, nullptr, nullptr) == TEASER_HIP_OK,
           "an ignored radius / ref is not checked, and the handle works afterwards", -1);
  }
  teaser_hip_icp_destroy(h);
  std::printf("cases %d  mismatches %d\n", n_cases, g_bad);
  return g_bad ? 1 : 0;
}
