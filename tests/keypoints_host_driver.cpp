// Host-only check of ISS keypoint detection (tests/test_keypoints_host.py): csrc/icp.hip, csrc/icp_outlier.hip and
// csrc/icp_keypoints.hip compiled by g++ against the HIP stand-in header, with the SOURCE of the lane-independent device code --
// csrc/icp_iss_device.h (keys, gather, the ordered neighbourhood walk, saliency, suppression, resolution) and the ring
// kernel of csrc/kernels_outlier.hip for the resolution's self k-NN -- run one lane at a time (tests/hip_stub runs a
// launch sequentially), built with -fsanitize=address,undefined as a stand-alone program.  "Device" buffers are host
// allocations of exactly the size the host code asked for, so a descriptor, a key layout, a sorted range or an output
// layout that is sized or addressed wrongly is an AddressSanitizer report; masks, saliencies, counts and radii are
// compared bit for bit with tests/keypoints_reference.py, read from a text file.  The device sort is replaced by
// std::stable_sort behind launch_iss_sort; the kernels' shells (kernels_keypoints.hip: one call each) are restated in
// the launchers below.  The scan kernel's wave merge cannot be emulated one lane at a time: no query of these cases
// reaches the worklist (asserted).
//   keypoints_host_driver CASES.txt    exit code 0: every case equal and every refusal refused
// TEST INFRASTRUCTURE ONLY.
#include <numeric>

#include "icp_host_prelude.h"
#include "../teaser-plusplus_amd/csrc/kernels_outlier.hip"
#include "../teaser-plusplus_amd/csrc/icp.hip"
#include "../teaser-plusplus_amd/csrc/icp_outlier.hip"
#include "../teaser-plusplus_amd/csrc/icp_keypoints.hip"

namespace thip {

// ---- kernels_keypoints.hip: the sort behind one function, the shells restated on the same bodies ----
size_t iss_sort_temp_bytes(int64_t) { return 16; }

hipError_t launch_iss_sort(hipStream_t, void*, size_t, int64_t entries, int bits, const uint64_t* key,
                           const int32_t* iota, uint64_t* skey, int32_t* sidx) {
  const uint64_t mask = bits >= 64 ? ~0ull : ((1ull << bits) - 1);  // the radix sort reads the low `bits` bits only
  std::vector<int64_t> order((size_t)entries);
  std::iota(order.begin(), order.end(), (int64_t)0);
  std::stable_sort(order.begin(), order.end(),
                   [&](int64_t a, int64_t b) { return (key[a] & mask) < (key[b] & mask); });
  for (int64_t e = 0; e < entries; ++e) {
    skey[e] = key[order[(size_t)e]];
    sidx[e] = iota[order[(size_t)e]];
  }
  return hipSuccess;
}

void launch_iss_keys(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk, const double* d_pts,
                     int64_t total, uint64_t* d_key, int32_t* d_iota) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(iss_keys_body, dim3(n_blk), dim3(kIssBlock), 0, s, d_desc, d_blk_prob, d_pts, total, d_key, d_iota);
}

void launch_iss_gather(hipStream_t s, int64_t total, const double* d_pts, const int32_t* d_sidx, double* d_spts) {
  if (total <= 0) return;
  hipLaunchKernelGGL(iss_gather_body, dim3((unsigned)((2 * total + kIssBlock - 1) / kIssBlock)), dim3(kIssBlock), 0, s,
                     total, d_pts, d_sidx, d_spts);
}

void launch_iss_saliency(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                         const uint64_t* d_skey, const int32_t* d_sidx, const double* d_spts, double* d_sal,
                         int32_t* d_count) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(iss_saliency_body, dim3(n_blk), dim3(kIssBlock), 0, s, d_desc, d_blk_prob, d_skey, d_sidx, d_spts,
                     d_sal, d_count);
}

static void suppress_shell(const IssDesc* descs, const int32_t* blk_prob, int64_t total, const uint64_t* skey,
                           const int32_t* sidx, const double* spts, const double* sal, int32_t* count, uint8_t* keep,
                           int32_t* kept) {
  int p = 0;
  if (iss_suppress_body(descs, blk_prob, total, skey, sidx, spts, sal, count, keep, p)) ++kept[p];
}

void launch_iss_suppress(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk, int64_t total,
                         const uint64_t* d_skey, const int32_t* d_sidx, const double* d_spts, const double* d_sal,
                         int32_t* d_count, uint8_t* d_keep, int32_t* d_kept) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(suppress_shell, dim3(n_blk), dim3(kIssBlock), 0, s, d_desc, d_blk_prob, total, d_skey, d_sidx,
                     d_spts, d_sal, d_count, d_keep, d_kept);
}

void launch_iss_resolution(hipStream_t s, const IcpDesc* d_desc, const IcpKnnDesc* d_knn, const int32_t* d_tblk_prob,
                           int n_tblk, int batch, const double* d_d2, double* d_partials, double* d_res) {
  if (n_tblk <= 0) return;
  hipLaunchKernelGGL(iss_res_block_body, dim3((n_tblk + 255) / 256), dim3(256), 0, s, d_desc, d_knn, d_tblk_prob,
                     n_tblk, d_d2, d_partials);
  hipLaunchKernelGGL(iss_res_reduce_body, dim3((batch + 255) / 256), dim3(256), 0, s, d_desc, batch, d_partials, d_res);
}

}  // namespace thip

struct Case {
  int n = 0;
  teaser_icp_iss_params_c prm;
  std::vector<double> pts, sal, radii;
  std::vector<uint8_t> keep;
  std::vector<int32_t> count;
};

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n_cases = 0;
  if (std::fscanf(f, "%d", &n_cases) != 1) return 2;
  std::vector<Case> cases((size_t)n_cases);
  for (Case& c : cases) {
    c.n = (int)read_number(f);
    memset(&c.prm, 0, sizeof(c.prm));
    c.prm.salient_radius = read_number(f), c.prm.non_max_radius = read_number(f);
    c.prm.gamma_21 = read_number(f), c.prm.gamma_32 = read_number(f);
    c.prm.min_neighbors = (int32_t)read_number(f);
    read_numbers(f, c.pts, 3 * (size_t)c.n);
    c.keep.resize((size_t)c.n);
    for (uint8_t& k : c.keep) k = (uint8_t)read_number(f);
    read_numbers(f, c.sal, (size_t)c.n);
    c.count.resize(2 * (size_t)c.n);
    for (int32_t& k : c.count) k = (int32_t)read_number(f);
    read_numbers(f, c.radii, 3);
  }
  std::fclose(f);

  teaser_hip_icp* h = nullptr;
  if (teaser_hip_icp_create(0, &h) != TEASER_HIP_OK) return 2;
  const int B = n_cases;
  for (int subset = 0; subset < 4; ++subset)  // which optional outputs are asked for: bit 0 saliencies, bit 1 counts
    for (int pass = 0; pass < 2; ++pass) {    // pass 0: every case alone; pass 1: all of them in one batch
      if (pass == 0 && subset != 3) continue;
      for (int lo = 0; lo < B; lo += pass ? B : 1) {
        const int b = pass ? B : 1;
        std::vector<const double*> pp((size_t)b);
        std::vector<int32_t> n((size_t)b), kept((size_t)b, -1);
        std::vector<teaser_icp_iss_params_c> rec((size_t)b);
        std::vector<std::vector<double>> sal((size_t)b);
        std::vector<std::vector<uint8_t>> keep((size_t)b);
        std::vector<std::vector<int32_t>> cnt((size_t)b);
        std::vector<double*> ps((size_t)b);
        std::vector<uint8_t*> pk((size_t)b);
        std::vector<int32_t*> pc((size_t)b);
        std::vector<double> radii(3 * (size_t)b);
        for (int c = 0; c < b; ++c) {
          const Case& cs = cases[(size_t)(lo + c)];
          const size_t m = (size_t)cs.n;
          pp[c] = m ? cs.pts.data() : nullptr;
          n[c] = cs.n;
          rec[c] = cs.prm;
          sal[c].assign(m, -1.0), keep[c].assign(m, 7), cnt[c].assign(2 * m, -1);
          pk[c] = m ? keep[c].data() : nullptr;
          // in the batch every other cloud leaves out an optional output the call as a whole asks for
          ps[c] = m && (subset & 1) && !(pass && c % 2 == 1) ? sal[c].data() : nullptr;
          pc[c] = m && (subset & 2) && !(pass && c % 3 == 1) ? cnt[c].data() : nullptr;
        }
        expect(teaser_hip_icp_iss_keypoints_batch(h, b, pp.data(), n.data(), rec.data(), pk.data(), kept.data(),
                                                  (subset & 1) ? ps.data() : nullptr, (subset & 2) ? pc.data() : nullptr,
                                                  radii.data()) == 0,
               teaser_hip_icp_last_error(h), lo);
        int64_t fell = -1;
        teaser_hip_icp_get_option(h, "knn_fallbacks", &fell);
        expect(fell == 0, "a query reached the worklist (the scan kernel is not emulated)", lo);
        for (int c = 0; c < b; ++c) {
          const Case& cs = cases[(size_t)(lo + c)];
          expect(keep[c] == cs.keep, "mask", lo + c);
          expect(kept[c] == (int32_t)std::count(cs.keep.begin(), cs.keep.end(), 1), "keypoint count", lo + c);
          if (ps[c]) expect(same(sal[c], cs.sal, true), "saliencies", lo + c);
          if (pc[c]) expect(cnt[c] == cs.count, "counts", lo + c);
          expect(same(std::vector<double>(radii.begin() + 3 * c, radii.begin() + 3 * c + 3), cs.radii, true), "radii", lo + c);
        }
      }
    }

  // refusals: BAD_ARG, the argument and the cloud named, and the handle still works
  {
    const Case& cs = cases[0];
    const double* pp[2] = {cs.pts.data(), cs.pts.data()};
    std::vector<double> bad = cs.pts;
    bad[4] = NAN;
    const double* pbad[2] = {cs.pts.data(), bad.data()};
    const double* pnull[2] = {cs.pts.data(), nullptr};
    const int32_t n[2] = {cs.n, cs.n};
    std::vector<uint8_t> k0((size_t)cs.n), k1((size_t)cs.n);
    uint8_t* pk[2] = {k0.data(), k1.data()};
    uint8_t* pk_null[2] = {k0.data(), nullptr};
    int32_t kept[2];
    auto refused = [&](const double* const* pts, teaser_icp_iss_params_c r1, uint8_t* const* keep, const char* w1) {
      teaser_icp_iss_params_c rec[2] = {cs.prm, r1};
      const int32_t rc = teaser_hip_icp_iss_keypoints_batch(h, 2, pts, n, rec, keep, kept, nullptr, nullptr, nullptr);
      const std::string msg = teaser_hip_icp_last_error(h);
      expect(rc == TEASER_HIP_ERR_BAD_ARG && msg.find(w1) != std::string::npos && msg.find("problem 1") != std::string::npos,
             (std::string("refusal: ") + w1 + " / " + msg).c_str(), -1);
    };
    auto with = [&](auto edit) {
      teaser_icp_iss_params_c r;
      teaser_hip_icp_iss_params_default(&r);
      r.salient_radius = 0.3, r.non_max_radius = 0.2;
      edit(r);
      return r;
    };
    refused(pbad, cs.prm, pk, "points");
    refused(pnull, cs.prm, pk, "points");
    refused(pp, cs.prm, pk_null, "keep_out");
    refused(pp, with([](auto& r) { r.salient_radius = -0.1; }), pk, "salient_radius");
    refused(pp, with([](auto& r) { r.salient_radius = NAN; }), pk, "salient_radius");
    refused(pp, with([](auto& r) { r.salient_radius = INFINITY; }), pk, "salient_radius");
    refused(pp, with([](auto& r) { r.salient_radius = 1e200; }), pk, "salient_radius");
    refused(pp, with([](auto& r) { r.non_max_radius = -1.0; }), pk, "non_max_radius");
    refused(pp, with([](auto& r) { r.non_max_radius = NAN; }), pk, "non_max_radius");
    refused(pp, with([](auto& r) { r.non_max_radius = 1e200; }), pk, "non_max_radius");
    refused(pp, with([](auto& r) { r.gamma_21 = NAN; }), pk, "gamma_21");
    refused(pp, with([](auto& r) { r.gamma_32 = INFINITY; }), pk, "gamma_32");
    refused(pp, with([](auto& r) { r.min_neighbors = -1; }), pk, "min_neighbors");
    refused(pp, with([](auto& r) { r.reserved = 1; }), pk, "reserved");
    refused(pp, with([](auto& r) { r.salient_radius = 1e-9; }), pk, "salient_radius is too small");
    refused(pp, with([](auto& r) { r.non_max_radius = 1e-9; }), pk, "non_max_radius is too small");
    teaser_icp_iss_params_c rec[2] = {cs.prm, cs.prm};
    expect(teaser_hip_icp_iss_keypoints_batch(h, 2, pp, n, nullptr, pk, kept, nullptr, nullptr, nullptr) ==
                   TEASER_HIP_ERR_BAD_ARG &&
               std::string(teaser_hip_icp_last_error(h)).find("params") != std::string::npos,
           "refusal: params", -1);
    expect(teaser_hip_icp_iss_keypoints_batch(h, 2, pp, n, rec, pk, nullptr, nullptr, nullptr, nullptr) ==
                   TEASER_HIP_ERR_BAD_ARG &&
               std::string(teaser_hip_icp_last_error(h)).find("n_keypoints_out") != std::string::npos,
           "refusal: n_keypoints_out", -1);
    expect(teaser_hip_icp_iss_keypoints_batch(h, 2, pp, n, rec, pk, kept, nullptr, nullptr, nullptr) == TEASER_HIP_OK &&
               k0 == cs.keep && k1 == cs.keep,
           "the handle works after the refusals", -1);
  }
  teaser_hip_icp_destroy(h);
  std::printf("cases %d  mismatches %d\n", n_cases, g_bad);
  return g_bad ? 1 : 0;
}
