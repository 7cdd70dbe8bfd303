// Host-only check of boundary-point detection (tests/test_boundary_host.py): csrc/icp_boundary.hip, with icp.hip,
// icp_outlier.hip, icp_normals.hip and icp_fpfh.hip (whose pieces, passes and list launches the call uses), compiled by
// g++ against the HIP stand-in header (tests/hip_stub), built with -ffp-contract=off -fsanitize=address,undefined.  The
// boundary launcher is a serial loop over the functions of csrc/icp_boundary_device.h -- the text the kernel compiles --
// walking the block map exactly as the kernel does, with std::sort in place of the kernel's network; the search
// launchers are the brute-force stand-ins of tests/search_host_driver.cpp; the normals launchers write a fixed function
// of the point, which the case file's normals restate.  "Device" buffers are host allocations of exactly the size the
// host code asked for, so a descriptor, a piece, a list row or an output layout that is sized or addressed wrongly is an
// AddressSanitizer report; the mask, the bits of max_gap and the list lengths are compared for equality with those of
// tests/boundary_reference.py, read from a text file (hexadecimal floats).
//   boundary_host_driver CASES.txt    exit code 0: every case equal and every refusal refused
// TEST INFRASTRUCTURE ONLY.
#include <utility>

#include "icp_host_prelude.h"
#include "../teaser-plusplus_amd/csrc/icp.hip"
#include "../teaser-plusplus_amd/csrc/icp_outlier.hip"
#include "../teaser-plusplus_amd/csrc/icp_normals.hip"
#include "../teaser-plusplus_amd/csrc/icp_fpfh.hip"
#include "../teaser-plusplus_amd/csrc/icp_boundary.hip"

namespace thip {

// the launchers of icp_outlier.hip: not called by this program
void launch_icp_self_knn(hipStream_t, const IcpDesc*, const IcpKnnDesc*, const int32_t*, int, int, const double*,
                         const double*, const int32_t*, const int32_t*, int32_t*, double*, double*, int32_t*, int32_t*) {
  std::abort();
}
void launch_icp_statistical(hipStream_t, const IcpDesc*, const IcpKnnDesc*, const int32_t*, int, int, const double*,
                            double*, double*, uint8_t*, int32_t*) {
  std::abort();
}
void launch_icp_radius_count(hipStream_t, const IcpDesc*, const IcpKnnDesc*, const int32_t*, int, const double*,
                             const double*, const int32_t*, int32_t*, uint8_t*, int32_t*) {
  std::abort();
}

// The normals launchers: point x gets (x0 + 1, x1 - 2, x2 + 0.5) / its length (tests/test_boundary_host.py restates it).
static void fake_normals(const IcpDesc* desc, const IcpNormalDesc* nd, const int32_t* blk_prob, int n_blk,
                         const double* q, double* nrm) {
  for (int blk = 0; blk < n_blk; ++blk) {
    const int p = blk_prob[blk];
    const IcpDesc& d = desc[p];
    for (int lane = 0; lane < kIcpCovBlock; ++lane) {
      const int64_t i = (int64_t)(blk - d.blk_off) * kIcpCovBlock + lane;
      if (i >= d.n_t) continue;
      const double* x = q + 3 * (d.t_off + i);
      const double v[3] = {x[0] + 1.0, x[1] - 2.0, x[2] + 0.5};
      const double len = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
      for (int c = 0; c < 3; ++c) nrm[3 * (nd[p].nrm_off + i) + c] = v[c] / len;
    }
  }
}
void launch_icp_normals_hybrid(hipStream_t, const IcpDesc* desc, const IcpNormalDesc* nd, const int32_t* blk_prob,
                               int n_blk, int, const double* q, const double*, const int32_t*, const int32_t*,
                               double* nrm, double*, double*) {
  fake_normals(desc, nd, blk_prob, n_blk, q, nrm);
}
void launch_icp_normals_knn(hipStream_t, const IcpDesc* desc, const IcpKnnDesc*, const IcpNormalDesc* nd,
                            const int32_t* blk_prob, int n_blk, int, const double* q, const double*, const int32_t*,
                            const int32_t*, double* nrm, double*, double*, int32_t*, int32_t*) {
  fake_normals(desc, nd, blk_prob, n_blk, q, nrm);
}

// ---- the search stand-ins of tests/search_host_driver.cpp ------------------------------------------------------------
static std::vector<std::pair<double, int32_t>> sorted_row(const IcpDesc& d, int64_t i, const double* x, const double* q) {
  std::vector<std::pair<double, int32_t>> c;
  const double* a = x + 3 * (d.s_off + i);
  for (int32_t j = 0; j < d.n_t; ++j) {
    const double* b = q + 3 * (d.t_off + j);
    const double e0 = a[0] - b[0], e1 = a[1] - b[1], e2 = a[2] - b[2];
    c.emplace_back((e0 * e0 + e1 * e1) + e2 * e2, j);
  }
  std::sort(c.begin(), c.end());
  return c;
}

static void serve(const IcpDesc& d, const IcpSearchDesc& sd, int64_t i, const double* x, const double* q, int32_t* idx,
                  double* d2, const double* r2, int32_t* cnt) {
  const auto c = sorted_row(d, i, x, q);
  int m = std::min(sd.k, d.n_t);
  if (r2) {
    int inside = 0;
    while (inside < d.n_t && c[(size_t)inside].first < *r2) ++inside;
    m = std::min(m, inside);
    cnt[d.s_off + i] = m;
  }
  for (int t = 0; t < sd.k; ++t) {
    idx[sd.out_off + i * sd.k + t] = t < m ? c[(size_t)t].second : -1;
    d2[sd.out_off + i * sd.k + t] = t < m ? c[(size_t)t].first : INFINITY;
  }
}

void launch_icp_search_knn(hipStream_t, const IcpDesc* desc, const IcpSearchDesc* sd, const int32_t* blk_prob, int n_blk,
                           int top_k, const double* x, const double* q, const double*, const int32_t*, const int32_t*,
                           int32_t* idx, double* d2, int32_t* work, int32_t* work_count) {
  for (int blk = 0; blk < n_blk; ++blk) {
    const int p = blk_prob[blk];
    const IcpDesc& d = desc[p];
    for (int lane = 0; lane < kIcpCovBlock; ++lane) {
      const int64_t i = (int64_t)(blk - d.blk_off) * kIcpCovBlock + lane;
      if (i >= d.n_s) continue;
      if (std::min(sd[p].k, d.n_t) > top_k) std::abort();  // the capacity the launcher would pick is too small
      if (sd[p].ring_cap == 0 || i % 3 == 0) {
        const int32_t w = (*work_count)++;
        work[2 * (int64_t)w] = p;
        work[2 * (int64_t)w + 1] = (int32_t)i;
      } else {
        serve(d, sd[p], i, x, q, idx, d2, nullptr, nullptr);
      }
    }
  }
  for (int32_t w = 0; w < *work_count; ++w)
    serve(desc[work[2 * (int64_t)w]], sd[work[2 * (int64_t)w]], work[2 * (int64_t)w + 1], x, q, idx, d2, nullptr, nullptr);
}

// (the queries of this call ARE the data as given, so the stand-in needs no look through the sorted copy)
void launch_icp_search_hybrid(hipStream_t, const IcpDesc* desc, const IcpSearchDesc* sd, const int32_t* blk_prob,
                              int n_blk, int top_nn, const double* x, const double*, const int32_t*, const int32_t*,
                              int32_t* idx, double* d2, int32_t* cnt) {
  for (int blk = 0; blk < n_blk; ++blk) {
    const int p = blk_prob[blk];
    const IcpDesc& d = desc[p];
    if (sd[p].k > top_nn) std::abort();
    for (int lane = 0; lane < kIcpCovBlock; ++lane) {
      const int64_t i = (int64_t)(blk - d.blk_off) * kIcpCovBlock + lane;
      if (i < d.n_s) serve(d, sd[p], i, x, x, idx, d2, &d.r2, cnt);
    }
  }
}

// the launchers of kernels_fpfh.hip: not called by this program
void launch_icp_fpfh_spfh(hipStream_t, const IcpDesc*, const IcpSearchDesc*, const int32_t*, int, int, const double*,
                          const double*, const int32_t*, double*) {
  std::abort();
}
void launch_icp_fpfh(hipStream_t, const IcpDesc*, const IcpSearchDesc*, const int32_t*, int, int, const int32_t*,
                     const double*, const double*, double*) {
  std::abort();
}

// ---- the boundary launch, serially, on the device header's functions ---------------------------------------------------
void launch_icp_boundary(hipStream_t, const IcpDesc* desc, const IcpSearchDesc* sd, const IcpBoundaryDesc* bd,
                         const int32_t* blk_prob, int n_hyb, int n_knn, const double* q, const double* normals,
                         const int32_t* list_idx, uint8_t* mask, double* max_gap, int32_t* count, int32_t* n_boundary) {
  for (int blk = 0; blk < n_hyb + n_knn; ++blk) {
    const int p = blk_prob[blk];
    const int rel = blk < n_hyb ? blk : blk - n_hyb;
    const IcpDesc& d = desc[p];
    const int64_t i0 = (int64_t)(rel - d.blk_off) * kIcpCovBlock;
    if (i0 < 0 || i0 >= d.n_s) std::abort();  // a block outside its piece
    const double* P = q + 3 * d.t_off;
    const double* N = normals + 3 * d.t_off;
    for (int64_t i = i0; i < i0 + kIcpCovBlock && i < d.n_s; ++i) {
      const int64_t ci = (d.s_off - d.t_off) + i;
      const int32_t* idx = list_idx + sd[p].out_off + i * sd[p].k;
      const int m = fpfh_list_length(idx, sd[p].k);
      double u[3], v[3], gap = 0.0;
      if (!boundary_frame(N + 3 * ci, u, v)) {
        gap = NAN;
      } else if (m > 1) {
        std::vector<double> a;
        bool nan = false;
        for (int k = 1; k < m; ++k) {
          a.push_back(boundary_angle(P + 3 * ci, P + 3 * (int64_t)idx[k], u, v));
          nan = nan || std::isnan(a.back());
        }
        if ((int)a.size() > kBoundarySlots) std::abort();
        std::sort(a.begin(), a.end());
        gap = nan ? NAN : boundary_max_gap(a.data(), (int)a.size());
      }
      const bool is = boundary_is_boundary(gap, bd[p].threshold);
      mask[d.s_off + i] = is ? 1 : 0;
      if (max_gap) max_gap[d.s_off + i] = gap;
      if (count) count[d.s_off + i] = m;
      if (is) n_boundary[bd[p].cloud] += 1;
    }
  }
}

}  // namespace thip

struct Case {
  int n = 0, search = 0, max_nn = 0, estimated = 0;
  double radius = 0, thr = 0;
  std::vector<double> pts, nrm, gap;
  std::vector<int> mask, m;
};

static teaser_icp_normal_search_c record(int search, int max_nn, double radius) {
  teaser_icp_normal_search_c r;
  memset(&r, 0, sizeof(r));
  r.search = search, r.max_nn = max_nn, r.radius = radius;
  return r;
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
    c.radius = read_number(f), c.thr = read_number(f), c.estimated = (int)read_number(f);
    read_numbers(f, c.pts, 3 * (size_t)c.n);
    read_numbers(f, c.nrm, 3 * (size_t)c.n);
    read_numbers(f, c.mask, (size_t)c.n);
    read_numbers(f, c.gap, (size_t)c.n);
    read_numbers(f, c.m, (size_t)c.n);
  }
  std::fclose(f);

  teaser_hip_icp* h = nullptr;
  if (teaser_hip_icp_create(0, &h) != TEASER_HIP_OK) return 2;
  int64_t def_bytes = 0;
  if (teaser_hip_icp_get_option(h, "fpfh_list_bytes", &def_bytes) != TEASER_HIP_OK) return 2;
  const int B = n_cases;
  // three values of the list bound (the default: one pass; 7680: pieces of 64 points at max_nn 10, several passes; 1:
  // every piece one block and a pass of its own), the ring cap 0 with the first
  for (int64_t bound : {def_bytes, (int64_t)7680, (int64_t)1})
    for (int ring_cap : {4, 0}) {
      if (ring_cap == 0 && bound != def_bytes) continue;
      if (teaser_hip_icp_set_option(h, "fpfh_list_bytes", bound) != TEASER_HIP_OK) return 2;
      if (teaser_hip_icp_set_option(h, "knn_ring_cap", ring_cap) != TEASER_HIP_OK) return 2;
      for (int pass = 0; pass < 3; ++pass)  // 0: every case alone; 1: all of them in one batch; 2: the batch reversed
        for (int lo = 0; lo < B; lo += pass ? B : 1) {
          const int b = pass ? B : 1;
          auto which = [&](int c) { return pass == 2 ? B - 1 - c : lo + c; };
          std::vector<const double*> pp((size_t)b), pn((size_t)b);
          std::vector<int32_t> n((size_t)b), nb((size_t)b, -5);
          std::vector<double> thr((size_t)b);
          std::vector<teaser_icp_normal_search_c> rec((size_t)b), nrec((size_t)b);
          std::vector<std::vector<uint8_t>> mk((size_t)b);
          std::vector<std::vector<double>> gp((size_t)b), no((size_t)b);
          std::vector<std::vector<int32_t>> cn((size_t)b);
          std::vector<uint8_t*> pm((size_t)b);
          std::vector<double*> pg((size_t)b), po((size_t)b);
          std::vector<int32_t*> pc((size_t)b);
          for (int c = 0; c < b; ++c) {
            const Case& cs = cases[(size_t)which(c)];
            const size_t m = (size_t)cs.n;
            pp[c] = m ? cs.pts.data() : nullptr;
            pn[c] = m && !cs.estimated ? cs.nrm.data() : nullptr;
            n[c] = cs.n;
            thr[c] = cs.thr;
            rec[c] = record(cs.search, cs.max_nn, cs.radius);
            nrec[c] = cs.estimated ? record(c % 2, 5, 0.25) : record(0, 0, 0.0);
            if (cs.estimated) nrec[c].orient = c % 3;
            mk[c].assign(m, 7), gp[c].assign(m, -7.5), cn[c].assign(m, -7), no[c].assign(3 * m, -7.5);
            pm[c] = m ? mk[c].data() : nullptr;
            pg[c] = m && (pass == 0 || c % 2 == 0) ? gp[c].data() : nullptr;  // an optional output left out by some
            pc[c] = m && (pass == 0 || c % 3 != 2) ? cn[c].data() : nullptr;
            po[c] = m && (pass == 0 || c % 3 != 1) ? no[c].data() : nullptr;
          }
          expect(teaser_hip_icp_boundary_points_batch(h, b, pp.data(), pn.data(), n.data(), rec.data(), nrec.data(),
                                                      thr.data(), pm.data(), nb.data(), pg.data(), pc.data(),
                                                      po.data()) == TEASER_HIP_OK, teaser_hip_icp_last_error(h), lo);
          for (int c = 0; c < b; ++c) {
            const Case& cs = cases[(size_t)which(c)];
            int ones = 0;
            bool mask_ok = true, m_ok = true;
            for (int i = 0; i < cs.n; ++i) {
              mask_ok = mask_ok && mk[c][(size_t)i] == cs.mask[(size_t)i];
              ones += cs.mask[(size_t)i];
              if (pc[c]) m_ok = m_ok && cn[c][(size_t)i] == cs.m[(size_t)i];
            }
            expect(mask_ok, "mask", which(c));
            expect(nb[c] == ones, "n_boundary", which(c));
            expect(m_ok, "counts", which(c));
            if (pg[c]) expect(same(gp[c], cs.gap), "max_gap bits", which(c));
            if (po[c]) expect(same(no[c], cs.nrm), "normals_out", which(c));
          }
        }
    }
  if (teaser_hip_icp_set_option(h, "fpfh_list_bytes", def_bytes) != TEASER_HIP_OK) return 2;
  if (teaser_hip_icp_set_option(h, "knn_ring_cap", 4) != TEASER_HIP_OK) return 2;

  // refusals: BAD_ARG, the argument and the cloud named, and the handle still works
  {
    const Case* pc = nullptr;
    for (const Case& c : cases)
      if (c.n >= 60 && !c.estimated && !pc) pc = &c;
    if (!pc) return 2;
    const Case& cs = *pc;
    const double* pp[2] = {cs.pts.data(), cs.pts.data()};
    const double* nn[2] = {cs.nrm.data(), cs.nrm.data()};
    std::vector<double> bad_p = cs.pts, bad_n = cs.nrm;
    bad_p[4] = NAN, bad_n[7] = INFINITY;
    const double* p_bad[2] = {cs.pts.data(), bad_p.data()};
    const double* n_bad[2] = {bad_n.data(), cs.nrm.data()};
    const double* n_half[2] = {cs.nrm.data(), nullptr};
    const int32_t n[2] = {cs.n, cs.n}, n_neg[2] = {cs.n, -1};
    std::vector<uint8_t> m0((size_t)cs.n), m1((size_t)cs.n);
    uint8_t* pm[2] = {m0.data(), m1.data()};
    uint8_t* pm_half[2] = {m0.data(), nullptr};
    int32_t nb[2] = {0, 0};
    const double t_ok[2] = {cs.thr, cs.thr};
    const teaser_icp_normal_search_c ok = record(0, 10, 0.3);
    auto with = [&](int which, teaser_icp_normal_search_c r) {
      std::vector<teaser_icp_normal_search_c> v(2, ok);
      v[(size_t)which] = r;
      return v;
    };
    auto refused = [&](int32_t rc, const char* w1, const char* w2) {
      const std::string msg = teaser_hip_icp_last_error(h);
      expect(rc == TEASER_HIP_ERR_BAD_ARG && msg.find(w1) != std::string::npos && msg.find(w2) != std::string::npos,
             (std::string("refusal: ") + w1 + " / " + msg).c_str(), -1);
    };
    auto call = [&](const double* const* p, const double* const* nr, const int32_t* cnt,
                    const std::vector<teaser_icp_normal_search_c>& s, const teaser_icp_normal_search_c* ns,
                    const double* t, uint8_t* const* out) {
      return teaser_hip_icp_boundary_points_batch(h, 2, p, nr, cnt, s.data(), ns, t, out, nb, nullptr, nullptr, nullptr);
    };
    const std::vector<teaser_icp_normal_search_c> oks(2, ok);
    refused(call(p_bad, nn, n, oks, nullptr, t_ok, pm), "points has a non-finite", "problem 1");
    refused(call(pp, n_bad, n, oks, nullptr, t_ok, pm), "normals has a non-finite", "problem 0");
    refused(call(pp, nn, n_neg, oks, nullptr, t_ok, pm), "n must be", "problem 1");
    refused(call(nullptr, nn, n, oks, nullptr, t_ok, pm), "points is NULL", "problem 0");
    refused(call(pp, nn, n, with(1, record(2, 10, 0.3)), nullptr, t_ok, pm), "radius-only", "problem 1");
    refused(call(pp, nn, n, with(0, record(3, 10, 0.3)), nullptr, t_ok, pm), "search must be 0 or 1", "problem 0");
    refused(call(pp, nn, n, with(1, record(0, 1, 0.3)), nullptr, t_ok, pm), "max_nn must lie in [2, 100]", "problem 1");
    refused(call(pp, nn, n, with(0, record(1, 101, 0.3)), nullptr, t_ok, pm), "max_nn must lie", "problem 0");
    refused(call(pp, nn, n, with(1, record(0, 10, 0.0)), nullptr, t_ok, pm), "radius", "problem 1");
    refused(call(pp, nn, n, with(0, record(0, 10, NAN)), nullptr, t_ok, pm), "radius", "problem 0");
    refused(call(pp, nn, n, with(1, record(0, 10, 1e200)), nullptr, t_ok, pm), "radius", "problem 1");
    teaser_icp_normal_search_c o1 = ok, rsv = ok;
    o1.orient = 1, rsv.reserved = 3;
    refused(call(pp, nn, n, with(1, o1), nullptr, t_ok, pm), "orient must be 0", "problem 1");
    refused(call(pp, nn, n, with(0, rsv), nullptr, t_ok, pm), "reserved", "problem 0");
    for (double bad : {-1e-9, 360.0000001, (double)NAN, (double)INFINITY}) {
      const double t_bad[2] = {90.0, bad};
      refused(call(pp, nn, n, oks, nullptr, t_bad, pm), "angle_threshold", "problem 1");
    }
    refused(call(pp, n_half, n, oks, nullptr, t_ok, pm), "normals is NULL and normal_search", "problem 1");
    const teaser_icp_normal_search_c none[2] = {record(0, 0, 0.0), record(0, 0, 0.0)};
    refused(call(pp, nullptr, n, oks, none, t_ok, pm), "normals is NULL and normal_search", "problem 0");
    const teaser_icp_normal_search_c nbad[2] = {record(0, 0, 0.0), record(0, 2, 0.2)};
    refused(call(pp, n_half, n, oks, nbad, t_ok, pm), "normal_search", "problem 1");
    refused(call(pp, nn, n, oks, nullptr, t_ok, pm_half), "mask_out is NULL", "problem 1");
    refused(call(pp, nn, n, oks, nullptr, t_ok, nullptr), "mask_out is NULL", "problem 0");
    auto named = [&](int32_t rc, const char* w) {
      expect(rc == TEASER_HIP_ERR_BAD_ARG && std::string(teaser_hip_icp_last_error(h)).find(w) != std::string::npos,
             (std::string("refusal: ") + w).c_str(), -1);
    };
    named(teaser_hip_icp_boundary_points_batch(h, 2, pp, nn, n, nullptr, nullptr, t_ok, pm, nb, nullptr, nullptr, nullptr),
          "search must not be NULL");
    named(teaser_hip_icp_boundary_points_batch(h, 2, pp, nn, n, oks.data(), nullptr, nullptr, pm, nb, nullptr, nullptr,
                                               nullptr), "angle_threshold must not be NULL");
    named(teaser_hip_icp_boundary_points_batch(h, 2, pp, nn, n, oks.data(), nullptr, t_ok, pm, nullptr, nullptr, nullptr,
                                               nullptr), "n_boundary_out must not be NULL");
    expect(teaser_hip_icp_boundary_points_batch(h, -1, pp, nn, n, oks.data(), nullptr, t_ok, pm, nb, nullptr, nullptr,
                                                nullptr) == TEASER_HIP_ERR_BAD_ARG, "refusal: batch", -1);
    expect(teaser_hip_icp_boundary_points_batch(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_OK, "an empty batch", -1);
    std::vector<teaser_icp_normal_search_c> own(2, record(cs.search, cs.max_nn, cs.radius));
    expect(call(pp, nn, n, own, nullptr, t_ok, pm) == TEASER_HIP_OK, "the handle works afterwards", -1);
    bool equal = nb[0] == nb[1];
    for (int i = 0; i < cs.n; ++i) equal = equal && m0[(size_t)i] == cs.mask[(size_t)i] && m1[(size_t)i] == cs.mask[(size_t)i];
    expect(equal, "two copies of a cloud agree with the restatement", -1);
  }
  teaser_hip_icp_destroy(h);
  std::printf("cases %d  mismatches %d\n", n_cases, g_bad);
  return g_bad ? 1 : 0;
}
