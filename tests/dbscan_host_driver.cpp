// Host-only check of DBSCAN clustering (tests/test_dbscan_host.py): csrc/icp.hip and csrc/icp_cluster.hip compiled by
// g++ against the HIP stand-in header, with the SOURCE of the lane-independent device code -- csrc/icp_iss_device.h
// (keys, gather, the ordered neighbourhood walk) and csrc/icp_dbscan_device.h (count, union, flatten, label and the
// union-find) -- run one lane at a time (tests/hip_stub runs a launch sequentially), built with
// -fsanitize=address,undefined as a stand-alone program.  "Device" buffers are host allocations of exactly the size the
// host code asked for, so a descriptor, a key layout, a sorted range, a parent slot or an output layout that is sized or
// addressed wrongly is an AddressSanitizer report; labels, counts, roots and cluster counts are compared with
// tests/dbscan_reference.py, read from a text file.  The device sort is replaced by std::stable_sort and the device scan
// by a loop; the compare-and-swap is a plain one (the stand-in has no atomics, and nothing here is concurrent); the
// kernels' shells (one call each) are restated in the launchers below.
//   dbscan_host_driver CASES.txt    exit code 0: every case equal and every refusal refused
// TEST INFRASTRUCTURE ONLY.
#include <numeric>

#include "icp_host_prelude.h"

#define THIP_DBSCAN_HOST_ATOMICS
namespace thip {
inline int32_t dbscan_load(const int32_t* a) { return *a; }
inline void dbscan_store(int32_t* a, int32_t v) { *a = v; }
inline int32_t dbscan_cas(int32_t* a, int32_t expect, int32_t v) {
  const int32_t old = *a;
  if (old == expect) *a = v;
  return old;
}
}  // namespace thip

#include "../teaser-plusplus_amd/csrc/icp.hip"
#include "../teaser-plusplus_amd/csrc/icp_cluster.hip"

namespace thip {

static int g_union_checks = 0;

// ---- kernels_keypoints.hip / kernels_cluster.hip: sort and scan behind one function each, the shells restated ----
size_t iss_sort_temp_bytes(int64_t) { return 16; }
size_t dbscan_scan_temp_bytes(int64_t) { return 8; }

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

hipError_t launch_dbscan_scan(hipStream_t, void*, size_t, int64_t entries, const int32_t* flag, int32_t* scan) {
  int32_t sum = 0;
  for (int64_t e = 0; e < entries; ++e) {
    scan[e] = sum;
    sum += flag[e];
  }
  return hipSuccess;
}

void launch_iss_keys_grids(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                           const double* d_pts, int64_t total, int grids, uint64_t* d_key, int32_t* d_iota) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(iss_keys_grids_body, dim3(n_blk), dim3(kIssBlock), 0, s, d_desc, d_blk_prob, d_pts, total, grids,
                     d_key, d_iota);
}

void launch_iss_gather_entries(hipStream_t s, int64_t total, int64_t entries, const double* d_pts,
                               const int32_t* d_sidx, double* d_spts) {
  if (entries <= 0) return;
  hipLaunchKernelGGL(iss_gather_entries_body, dim3((unsigned)((entries + kIssBlock - 1) / kIssBlock)), dim3(kIssBlock),
                     0, s, total, entries, d_pts, d_sidx, d_spts);
}

void launch_dbscan_count(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                         const uint64_t* d_skey, const int32_t* d_sidx, const double* d_spts, int32_t* d_count,
                         int32_t* d_parent) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(dbscan_count_body, dim3(n_blk), dim3(kIssBlock), 0, s, d_desc, d_blk_prob, d_skey, d_sidx, d_spts,
                     d_count, d_parent);
}

void launch_dbscan_union(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                         const uint64_t* d_skey, const int32_t* d_sidx, const double* d_spts, const int32_t* d_count,
                         int32_t* d_parent) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(dbscan_union_body, dim3(n_blk), dim3(kIssBlock), 0, s, d_desc, d_blk_prob, d_skey, d_sidx, d_spts,
                     d_count, d_parent);
  // the invariant of the union-find after the kernel: parent[g] <= g inside every active cloud
  for (int b = 0; b < n_blk; ++b) {
    const IssDesc& d = d_desc[d_blk_prob[b]];
    if (!d.active) continue;
    for (int64_t g = d.off; g < d.off + d.n; ++g) {
      if (d_parent[g] > g || d_parent[g] < d.off) {
        std::fprintf(stderr, "parent[%lld] = %d breaks the invariant\n", (long long)g, d_parent[g]);
        ++g_bad;
      }
      ++g_union_checks;
    }
  }
}

void launch_dbscan_flatten(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                           const int32_t* d_count, const int32_t* d_parent, int32_t* d_root, int32_t* d_is_root) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(dbscan_flatten_body, dim3(n_blk), dim3(kIssBlock), 0, s, d_desc, d_blk_prob, d_count, d_parent,
                     d_root, d_is_root);
}

void launch_dbscan_label(hipStream_t s, const IssDesc* d_desc, const int32_t* d_blk_prob, int n_blk,
                         const uint64_t* d_skey, const int32_t* d_sidx, const double* d_spts, const int32_t* d_root,
                         const int32_t* d_scan, int32_t* d_label, int32_t* d_n_clusters) {
  if (n_blk <= 0) return;
  hipLaunchKernelGGL(dbscan_label_body, dim3(n_blk), dim3(kIssBlock), 0, s, d_desc, d_blk_prob, d_skey, d_sidx, d_spts,
                     d_root, d_scan, d_label, d_n_clusters);
}

}  // namespace thip

struct Case {
  int n = 0;
  teaser_icp_dbscan_params_c prm;
  int32_t c = 0;
  std::vector<double> pts;
  std::vector<int32_t> labels, count, root;
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
    c.prm.eps = read_number(f);
    c.prm.min_points = (int32_t)read_number(f);
    c.c = (int32_t)read_number(f);
    read_numbers(f, c.pts, 3 * (size_t)c.n);
    read_numbers(f, c.labels, (size_t)c.n);
    read_numbers(f, c.count, (size_t)c.n);
    read_numbers(f, c.root, (size_t)c.n);
  }
  std::fclose(f);

  teaser_hip_icp* h = nullptr;
  if (teaser_hip_icp_create(0, &h) != TEASER_HIP_OK) return 2;
  const int B = n_cases;
  for (int subset = 0; subset < 4; ++subset)  // which optional outputs are asked for: bit 0 counts, bit 1 roots
    for (int pass = 0; pass < 3; ++pass) {    // 0: every case alone; 1: all in one batch; 2: the batch in reverse order
      if (pass == 0 && subset != 3) continue;
      for (int lo = 0; lo < B; lo += pass ? B : 1) {
        const int b = pass ? B : 1;
        std::vector<const double*> pp((size_t)b);
        std::vector<int32_t> n((size_t)b), ncl((size_t)b, -7);
        std::vector<teaser_icp_dbscan_params_c> rec((size_t)b);
        std::vector<std::vector<int32_t>> lab((size_t)b), cnt((size_t)b), root((size_t)b);
        std::vector<int32_t*> pl((size_t)b), pc((size_t)b), pr((size_t)b);
        std::vector<int> which((size_t)b);
        for (int c = 0; c < b; ++c) {
          which[c] = pass == 2 ? B - 1 - c : lo + c;
          const Case& cs = cases[(size_t)which[c]];
          const size_t m = (size_t)cs.n;
          pp[c] = m ? cs.pts.data() : nullptr;
          n[c] = cs.n;
          rec[c] = cs.prm;
          lab[c].assign(m, -7), cnt[c].assign(m, -7), root[c].assign(m, -7);
          pl[c] = m ? lab[c].data() : nullptr;
          // in the batch every other cloud leaves out an optional output the call as a whole asks for
          pc[c] = m && (subset & 1) && !(pass && c % 2 == 1) ? cnt[c].data() : nullptr;
          pr[c] = m && (subset & 2) && !(pass && c % 3 == 1) ? root[c].data() : nullptr;
        }
        expect(teaser_hip_icp_cluster_dbscan_batch(h, b, pp.data(), n.data(), rec.data(), pl.data(), ncl.data(),
                                                   (subset & 1) ? pc.data() : nullptr,
                                                   (subset & 2) ? pr.data() : nullptr) == 0,
               teaser_hip_icp_last_error(h), lo);
        for (int c = 0; c < b; ++c) {
          const Case& cs = cases[(size_t)which[c]];
          expect(lab[c] == cs.labels, "labels", which[c]);
          expect(ncl[c] == cs.c, "cluster count", which[c]);
          if (pc[c]) expect(cnt[c] == cs.count, "counts", which[c]);
          if (pr[c]) expect(root[c] == cs.root, "roots", which[c]);
          if (!pc[c]) expect(cnt[c] == std::vector<int32_t>((size_t)cs.n, -7), "counts were not asked for", which[c]);
          if (!pr[c]) expect(root[c] == std::vector<int32_t>((size_t)cs.n, -7), "roots were not asked for", which[c]);
        }
      }
    }
  expect(thip::g_union_checks > 0, "the union-find invariant was checked", -1);

  // refusals: BAD_ARG, the argument and the cloud named, and the handle still works
  {
    const Case& cs = cases[0];
    const double* pp[2] = {cs.pts.data(), cs.pts.data()};
    std::vector<double> bad = cs.pts;
    bad[4] = NAN;
    std::vector<double> wide = cs.pts;  // an extent of 1e6
    wide[0] += 1e6;
    const double* pbad[2] = {cs.pts.data(), bad.data()};
    const double* pnull[2] = {cs.pts.data(), nullptr};
    const double* pwide[2] = {cs.pts.data(), wide.data()};
    const int32_t n[2] = {cs.n, cs.n};
    std::vector<int32_t> l0((size_t)cs.n), l1((size_t)cs.n);
    int32_t* pl[2] = {l0.data(), l1.data()};
    int32_t* pl_null[2] = {l0.data(), nullptr};
    int32_t ncl[2];
    auto refused = [&](const double* const* pts, teaser_icp_dbscan_params_c r1, int32_t* const* labels, const char* w1) {
      teaser_icp_dbscan_params_c rec[2] = {cs.prm, r1};
      const int32_t rc = teaser_hip_icp_cluster_dbscan_batch(h, 2, pts, n, rec, labels, ncl, nullptr, nullptr);
      const std::string msg = teaser_hip_icp_last_error(h);
      expect(rc == TEASER_HIP_ERR_BAD_ARG && msg.find(w1) != std::string::npos && msg.find("problem 1") != std::string::npos,
             (std::string("refusal: ") + w1 + " / " + msg).c_str(), -1);
    };
    auto with = [&](auto edit) {
      teaser_icp_dbscan_params_c r = cs.prm;
      edit(r);
      return r;
    };
    refused(pbad, cs.prm, pl, "points");
    refused(pnull, cs.prm, pl, "points");
    refused(pp, cs.prm, pl_null, "labels_out");
    refused(pp, with([](auto& r) { r.eps = -0.1; }), pl, "eps");
    refused(pp, with([](auto& r) { r.eps = NAN; }), pl, "eps");
    refused(pp, with([](auto& r) { r.eps = INFINITY; }), pl, "eps");
    refused(pp, with([](auto& r) { r.eps = 1e200; }), pl, "eps");
    refused(pp, with([](auto& r) { r.min_points = 0; }), pl, "min_points");
    refused(pp, with([](auto& r) { r.min_points = -3; }), pl, "min_points");
    refused(pp, with([](auto& r) { r.reserved = 1; }), pl, "reserved");
    refused(pwide, with([](auto& r) { r.eps = 1e-7; }), pl, "eps is too small");
    teaser_icp_dbscan_params_c rec[2] = {cs.prm, cs.prm};
    expect(teaser_hip_icp_cluster_dbscan_batch(nullptr, 2, pp, n, rec, pl, ncl, nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG,
           "refusal: handle", -1);
    expect(teaser_hip_icp_cluster_dbscan_batch(h, -1, pp, n, rec, pl, ncl, nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG &&
               std::string(teaser_hip_icp_last_error(h)).find("batch") != std::string::npos,
           "refusal: batch", -1);
    expect(teaser_hip_icp_cluster_dbscan_batch(h, 2, pp, nullptr, rec, pl, ncl, nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG &&
               std::string(teaser_hip_icp_last_error(h)).find("n must") != std::string::npos,
           "refusal: n", -1);
    expect(teaser_hip_icp_cluster_dbscan_batch(h, 2, pp, n, nullptr, pl, ncl, nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG &&
               std::string(teaser_hip_icp_last_error(h)).find("params") != std::string::npos,
           "refusal: params", -1);
    expect(teaser_hip_icp_cluster_dbscan_batch(h, 2, pp, n, rec, nullptr, ncl, nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG &&
               std::string(teaser_hip_icp_last_error(h)).find("labels_out") != std::string::npos,
           "refusal: labels_out", -1);
    expect(teaser_hip_icp_cluster_dbscan_batch(h, 2, pp, n, rec, pl, nullptr, nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG &&
               std::string(teaser_hip_icp_last_error(h)).find("n_clusters_out") != std::string::npos,
           "refusal: n_clusters_out", -1);
    expect(teaser_hip_icp_cluster_dbscan_batch(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
               TEASER_HIP_OK,
           "an empty batch is legal", -1);
    expect(teaser_hip_icp_cluster_dbscan_batch(h, 2, pp, n, rec, pl, ncl, nullptr, nullptr) == TEASER_HIP_OK &&
               l0 == cs.labels && l1 == cs.labels && ncl[0] == cs.c && ncl[1] == cs.c,
           "the handle works after the refusals", -1);
  }
  teaser_hip_icp_destroy(h);
  std::printf("cases %d  mismatches %d\n", n_cases, g_bad);
  return g_bad ? 1 : 0;
}
