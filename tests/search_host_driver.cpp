// Host-only check of the neighbour-search entry points (tests/test_search_host.py): csrc/icp_search.hip, with icp.hip and
// icp_outlier.hip, compiled by g++ against the HIP stand-in header (tests/hip_stub) with CPU stand-ins for the kernel
// launchers, built with -fsanitize=address,undefined.  "Device" buffers are host allocations of exactly the size the host
// code asked for, so a descriptor, an output layout, a worklist or a temporary that is sized or addressed wrongly is an
// AddressSanitizer report; the results are compared for equality with the numbers of tests/search_reference.py, read
// from a text file.
//   search_host_driver CASES.txt    exit code 0: every case equal and every refusal refused
// TEST INFRASTRUCTURE ONLY.
#include <utility>

#include "icp_host_prelude.h"
#include "../teaser-plusplus_amd/csrc/icp.hip"
#include "../teaser-plusplus_amd/csrc/icp_outlier.hip"
#include "../teaser-plusplus_amd/csrc/icp_search.hip"

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

// (the stand-ins below look through the data points themselves, not the index; the data as given lie in q at t_off,
// the queries in x at s_off)
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

// Every block of the launch is visited through the block map, as the kernel does; a query without data is served at
// once, every third other query (all of them when the ring cap is 0) goes through the worklist.
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
      if (d.n_t > 0 && (sd[p].ring_cap == 0 || i % 3 == 0)) {
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

// The stand-ins of the two radius-grid launchers read the data as given through the sorted copy's index: qs / qj hold
// every point of the cloud once.
static std::vector<double> unsorted(const IcpDesc* desc, int batch, const double* qs, const int32_t* qj) {
  int64_t total = 0;
  for (int p = 0; p < batch; ++p) total += desc[p].n_t;
  std::vector<double> q(3 * (size_t)total + 1);
  for (int p = 0; p < batch; ++p)
    for (int64_t s = desc[p].t_off; s < desc[p].t_off + desc[p].n_t; ++s)
      for (int c = 0; c < 3; ++c) q[(size_t)(3 * (desc[p].t_off + qj[s]) + c)] = qs[3 * s + c];
  return q;
}

void launch_icp_search_hybrid(hipStream_t, const IcpDesc* desc, const IcpSearchDesc* sd, const int32_t* blk_prob,
                              int n_blk, int top_nn, const double* x, const double* qs, const int32_t* qj,
                              const int32_t*, int32_t* idx, double* d2, int32_t* cnt) {
  int batch = 0;
  for (int blk = 0; blk < n_blk; ++blk) batch = std::max(batch, blk_prob[blk] + 1);
  const std::vector<double> q = unsorted(desc, batch, qs, qj);
  for (int blk = 0; blk < n_blk; ++blk) {
    const int p = blk_prob[blk];
    const IcpDesc& d = desc[p];
    if (sd[p].k > top_nn) std::abort();
    for (int lane = 0; lane < kIcpCovBlock; ++lane) {
      const int64_t i = (int64_t)(blk - d.blk_off) * kIcpCovBlock + lane;
      if (i < d.n_s) serve(d, sd[p], i, x, q.data(), idx, d2, &d.r2, cnt);
    }
  }
}

void launch_icp_search_radius(hipStream_t, const IcpDesc* desc, const IcpSearchDesc* sd, const int32_t* blk_prob,
                              int n_blk, int batch, int64_t entries, const double* x, const double* qs,
                              const int32_t* qj, const int32_t*, int32_t* count, int64_t* prefix, int64_t* total,
                              double* tmp_d2, int32_t* tmp_j, int32_t* idx, double* d2) {
  const std::vector<double> q = unsorted(desc, batch, qs, qj);
  for (int p = 0; p < batch; ++p) total[p] = 0;
  for (int blk = 0; blk < n_blk; ++blk) {
    const int p = blk_prob[blk];
    const IcpDesc& d = desc[p];
    for (int t = 0; t < 256; ++t) {
      const int64_t i = (int64_t)(blk - d.blk_off) * 256 + t;
      if (i >= d.n_s) continue;
      const auto c = sorted_row(d, i, x, q.data());
      int32_t inside = 0;
      while (inside < d.n_t && c[(size_t)inside].first < d.r2) ++inside;
      count[d.s_off + i] = inside;
    }
  }
  for (int p = 0; p < batch; ++p)
    for (int64_t i = 0; i < desc[p].n_s; ++i) {
      prefix[desc[p].s_off + i] = total[p];
      total[p] += count[desc[p].s_off + i];
    }
  if (entries <= 0) return;
  for (int p = 0; p < batch; ++p) {
    const IcpDesc& d = desc[p];
    if (!sd[p].fill || sd[p].capacity < total[p]) continue;
    const int64_t reserved = (p + 1 < batch ? sd[p + 1].out_off : entries) - sd[p].out_off;
    if (total[p] > reserved) std::abort();  // the host reserved too little
    for (int64_t i = 0; i < d.n_s; ++i) {
      const auto c = sorted_row(d, i, x, q.data());
      const int64_t at = sd[p].out_off + prefix[d.s_off + i];
      const int32_t m = count[d.s_off + i];
      for (int32_t t = 0; t < m; ++t) {
        tmp_d2[at + (m - 1 - t)] = c[(size_t)t].first;  // the temporary takes the row in another order
        tmp_j[at + (m - 1 - t)] = c[(size_t)t].second;
        idx[at + t] = c[(size_t)t].second;
        d2[at + t] = c[(size_t)t].first;
      }
    }
  }
}

}  // namespace thip

struct Case {
  int n_d = 0, n_q = 0, k = 0, max_nn = 0;
  double radius = 0;
  std::vector<double> data, query, k_d2, h_d2, r_d2;
  std::vector<int32_t> k_idx, h_idx, h_cnt, r_cnt, r_idx;
};

static const int32_t kSentinelI = -77;
static const double kSentinelD = -77.5;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n_cases = 0;
  if (std::fscanf(f, "%d", &n_cases) != 1) return 2;
  std::vector<Case> cases((size_t)n_cases);
  for (Case& c : cases) {
    c.n_d = (int)read_number(f), c.n_q = (int)read_number(f), c.k = (int)read_number(f);
    c.radius = read_number(f), c.max_nn = (int)read_number(f);
    const size_t total = (size_t)read_number(f), nq = (size_t)c.n_q;
    read_numbers(f, c.data, 3 * (size_t)c.n_d);
    read_numbers(f, c.query, 3 * nq);
    read_numbers(f, c.k_idx, nq * (size_t)c.k);
    read_numbers(f, c.k_d2, nq * (size_t)c.k);
    read_numbers(f, c.h_idx, nq * (size_t)c.max_nn);
    read_numbers(f, c.h_d2, nq * (size_t)c.max_nn);
    read_numbers(f, c.h_cnt, nq);
    read_numbers(f, c.r_cnt, nq);
    read_numbers(f, c.r_idx, total);
    read_numbers(f, c.r_d2, total);
  }
  std::fclose(f);

  teaser_hip_icp* h = nullptr;
  if (teaser_hip_icp_create(0, &h) != TEASER_HIP_OK) return 2;
  const int B = n_cases;
  for (int ring_cap : {4, 0}) {
    if (teaser_hip_icp_set_option(h, "knn_ring_cap", ring_cap) != TEASER_HIP_OK) return 2;
    for (int pass = 0; pass < 3; ++pass) {  // 0: every case alone; 1: all of them in one batch; 2: the batch reversed
      for (int lo = 0; lo < B; lo += pass ? B : 1) {
        const int b = pass ? B : 1;
        auto which = [&](int c) { return pass == 2 ? B - 1 - c : lo + c; };
        std::vector<const double*> pd((size_t)b), pq((size_t)b);
        std::vector<int32_t> nd((size_t)b), nq((size_t)b), k((size_t)b), nn((size_t)b);
        std::vector<double> radius((size_t)b);
        std::vector<std::vector<int32_t>> kidx((size_t)b), hidx((size_t)b), hcnt((size_t)b), rcnt((size_t)b), ridx((size_t)b);
        std::vector<std::vector<double>> kd2((size_t)b), hd2((size_t)b), rd2((size_t)b);
        std::vector<int32_t*> pki((size_t)b), phi((size_t)b), phc((size_t)b), prc((size_t)b), pri((size_t)b);
        std::vector<double*> pkd((size_t)b), phd((size_t)b), prd((size_t)b);
        std::vector<int64_t> cap((size_t)b), total((size_t)b, -1);
        int64_t queries_with_data = 0;
        for (int c = 0; c < b; ++c) {
          const Case& cs = cases[(size_t)which(c)];
          const size_t m = (size_t)cs.n_q;
          pd[c] = cs.n_d ? cs.data.data() : nullptr;  // an empty side passes NULL everywhere
          pq[c] = m ? cs.query.data() : nullptr;
          nd[c] = cs.n_d, nq[c] = cs.n_q, k[c] = cs.k, nn[c] = cs.max_nn, radius[c] = cs.radius;
          kidx[c].resize(m * (size_t)cs.k), kd2[c].resize(m * (size_t)cs.k);
          hidx[c].resize(m * (size_t)cs.max_nn), hd2[c].resize(m * (size_t)cs.max_nn), hcnt[c].resize(m), rcnt[c].resize(m);
          pki[c] = m ? kidx[c].data() : nullptr, pkd[c] = m ? kd2[c].data() : nullptr;
          phi[c] = m ? hidx[c].data() : nullptr, phd[c] = m ? hd2[c].data() : nullptr, phc[c] = m ? hcnt[c].data() : nullptr;
          prc[c] = m ? rcnt[c].data() : nullptr;
          if (cs.n_d) queries_with_data += cs.n_q;
        }
        int64_t fell = -1;
        expect(teaser_hip_icp_knn_search_batch(h, b, pd.data(), nd.data(), pq.data(), nq.data(), k.data(), pki.data(), pkd.data()) == 0, "knn rc", lo);
        teaser_hip_icp_get_option(h, "knn_fallbacks", &fell);
        expect(ring_cap == 0 ? fell == queries_with_data : fell <= queries_with_data, "knn_fallbacks", lo);
        expect(teaser_hip_icp_hybrid_search_batch(h, b, pd.data(), nd.data(), pq.data(), nq.data(), radius.data(), nn.data(), phi.data(), phd.data(), phc.data()) == 0, "hybrid rc", lo);
        teaser_hip_icp_get_option(h, "knn_fallbacks", &fell);
        expect(fell == 0, "hybrid leaves knn_fallbacks at 0", lo);
        for (int c = 0; c < b; ++c) {
          const Case& cs = cases[(size_t)which(c)];
          expect(kidx[c] == cs.k_idx, "knn idx", which(c));
          expect(same(kd2[c], cs.k_d2), "knn d2", which(c));
          expect(hidx[c] == cs.h_idx && hcnt[c] == cs.h_cnt, "hybrid idx / count", which(c));
          expect(same(hd2[c], cs.h_d2), "hybrid d2", which(c));
        }
        // the radius search in its halves: 0 count only (no arrays at all); 1 arrays one entry short (and a problem
        // without entries exact); 2 exact; 3 every other problem short, the others with room to spare
        for (int half = 0; half < 4; ++half) {
          for (int c = 0; c < b; ++c) {
            const Case& cs = cases[(size_t)which(c)];
            const int64_t tot = (int64_t)cs.r_idx.size();
            const bool short_ = half == 1 || (half == 3 && c % 2 == 0);
            cap[c] = half == 0 ? 0 : short_ ? std::max<int64_t>(tot - 1, 0) : tot + (half == 3 ? 5 : 0);
            ridx[c].assign((size_t)cap[c] + 1, kSentinelI), rd2[c].assign((size_t)cap[c] + 1, kSentinelD);
            pri[c] = ridx[c].data(), prd[c] = rd2[c].data();
            std::fill(rcnt[c].begin(), rcnt[c].end(), -5);
            total[c] = -1;
          }
          expect(teaser_hip_icp_radius_search_batch(h, b, pd.data(), nd.data(), pq.data(), nq.data(), radius.data(),
                                                    half ? cap.data() : nullptr, prc.data(), half ? pri.data() : nullptr,
                                                    half ? prd.data() : nullptr, total.data()) == 0, "radius rc", lo);
          teaser_hip_icp_get_option(h, "knn_fallbacks", &fell);
          expect(fell == 0, "radius leaves knn_fallbacks at 0", lo);
          for (int c = 0; c < b; ++c) {
            const Case& cs = cases[(size_t)which(c)];
            const size_t tot = cs.r_idx.size();
            expect(rcnt[c] == cs.r_cnt && total[c] == (int64_t)tot, "radius counts / total", which(c));
            const bool filled = half != 0 && cap[c] >= (int64_t)tot;
            std::vector<int32_t> want_i((size_t)cap[c] + 1, kSentinelI);
            std::vector<double> want_d((size_t)cap[c] + 1, kSentinelD);
            if (filled) {
              std::copy(cs.r_idx.begin(), cs.r_idx.end(), want_i.begin());
              std::copy(cs.r_d2.begin(), cs.r_d2.end(), want_d.begin());
            }
            expect(ridx[c] == want_i && same(rd2[c], want_d), filled ? "radius rows" : "radius arrays untouched", which(c));
          }
        }
      }
    }
  }
  // refusals: BAD_ARG, the argument and the problem named, and the handle still works
  {
    const Case& cs = cases[0];
    const double* pp[2] = {cs.data.data(), cs.data.data()};
    const double* qq[2] = {cs.query.data(), cs.query.data()};
    std::vector<double> bad_d = cs.data, bad_q = cs.query;
    bad_d[4] = NAN, bad_q[2] = INFINITY;
    const double* pbad[2] = {cs.data.data(), bad_d.data()};
    const double* qbad[2] = {bad_q.data(), cs.query.data()};
    const double* qnull[2] = {cs.query.data(), nullptr};
    const int32_t nd[2] = {cs.n_d, cs.n_d}, nq[2] = {cs.n_q, cs.n_q}, n_neg[2] = {cs.n_q, -1};
    std::vector<int32_t> i0((size_t)cs.n_q * 100), i1((size_t)cs.n_q * 100), c0((size_t)cs.n_q), c1((size_t)cs.n_q);
    int32_t* pi[2] = {i0.data(), i1.data()};
    int32_t* pi_half[2] = {i0.data(), nullptr};
    int32_t* pc[2] = {c0.data(), c1.data()};
    int32_t* pc_half[2] = {nullptr, c1.data()};
    int64_t total[2];
    auto refused = [&](int32_t rc, const char* w1, const char* w2) {
      const std::string msg = teaser_hip_icp_last_error(h);
      expect(rc == TEASER_HIP_ERR_BAD_ARG && msg.find(w1) != std::string::npos && msg.find(w2) != std::string::npos,
             (std::string("refusal: ") + w1 + " / " + msg).c_str(), -1);
    };
    const int32_t k_ok[2] = {5, 5}, k_lo[2] = {5, 0}, k_hi[2] = {101, 5};
    const double r_ok[2] = {0.2, 0.2}, r_zero[2] = {0.2, 0.0}, r_nan[2] = {NAN, 0.2}, r_big[2] = {0.1, 1e200};
    const double r_tiny[2] = {1e-200, 0.2};
    const int64_t cap_neg[2] = {10, -1};
    refused(teaser_hip_icp_knn_search_batch(h, 2, pbad, nd, qq, nq, k_ok, pi, nullptr), "data has a non-finite", "problem 1");
    refused(teaser_hip_icp_knn_search_batch(h, 2, pp, nd, qbad, nq, k_ok, pi, nullptr), "query has a non-finite", "problem 0");
    refused(teaser_hip_icp_knn_search_batch(h, 2, pp, nd, qnull, nq, k_ok, pi, nullptr), "query is NULL", "problem 1");
    refused(teaser_hip_icp_knn_search_batch(h, 2, nullptr, nd, qq, nq, k_ok, pi, nullptr), "data is NULL", "problem 0");
    refused(teaser_hip_icp_knn_search_batch(h, 2, pp, nd, qq, n_neg, k_ok, pi, nullptr), "n_query", "problem 1");
    refused(teaser_hip_icp_knn_search_batch(h, 2, pp, n_neg, qq, nq, k_ok, pi, nullptr), "n_data", "problem 1");
    refused(teaser_hip_icp_knn_search_batch(h, 2, pp, nd, qq, nq, k_lo, pi, nullptr), "k must lie", "problem 1");
    refused(teaser_hip_icp_knn_search_batch(h, 2, pp, nd, qq, nq, k_hi, pi, nullptr), "k must lie", "problem 0");
    refused(teaser_hip_icp_knn_search_batch(h, 2, pp, nd, qq, nq, k_ok, pi_half, nullptr), "idx_out", "problem 1");
    refused(teaser_hip_icp_knn_search_batch(h, 2, pp, nd, qq, nq, k_ok, nullptr, nullptr), "idx_out", "problem 0");
    refused(teaser_hip_icp_hybrid_search_batch(h, 2, pp, nd, qq, nq, r_zero, k_ok, pi, nullptr, nullptr), "radius", "problem 1");
    refused(teaser_hip_icp_hybrid_search_batch(h, 2, pp, nd, qq, nq, r_nan, k_ok, pi, nullptr, nullptr), "radius", "problem 0");
    refused(teaser_hip_icp_hybrid_search_batch(h, 2, pp, nd, qq, nq, r_big, k_ok, pi, nullptr, nullptr), "radius", "problem 1");
    refused(teaser_hip_icp_hybrid_search_batch(h, 2, pp, nd, qq, nq, r_tiny, k_ok, pi, nullptr, nullptr), "radius", "problem 0");
    refused(teaser_hip_icp_hybrid_search_batch(h, 2, pp, nd, qq, nq, r_ok, k_hi, pi, nullptr, nullptr), "max_nn must lie", "problem 0");
    refused(teaser_hip_icp_hybrid_search_batch(h, 2, pp, nd, qq, nq, r_ok, k_lo, pi, nullptr, nullptr), "max_nn must lie", "problem 1");
    refused(teaser_hip_icp_hybrid_search_batch(h, 2, pbad, nd, qq, nq, r_ok, k_ok, pi, nullptr, nullptr), "data has a non-finite", "problem 1");
    refused(teaser_hip_icp_hybrid_search_batch(h, 2, pp, nd, qq, nq, r_ok, k_ok, pi_half, nullptr, nullptr), "idx_out", "problem 1");
    refused(teaser_hip_icp_radius_search_batch(h, 2, pp, nd, qq, nq, r_zero, nullptr, pc, nullptr, nullptr, total), "radius", "problem 1");
    refused(teaser_hip_icp_radius_search_batch(h, 2, pp, nd, qbad, nq, r_ok, nullptr, pc, nullptr, nullptr, total), "query has a non-finite", "problem 0");
    refused(teaser_hip_icp_radius_search_batch(h, 2, pp, nd, qq, nq, r_ok, nullptr, pc_half, nullptr, nullptr, total), "count_out", "problem 0");
    refused(teaser_hip_icp_radius_search_batch(h, 2, pp, nd, qq, nq, r_ok, cap_neg, pc, pi, nullptr, total), "capacity", "problem 1");
    refused(teaser_hip_icp_radius_search_batch(h, 2, pp, nd, qq, nq, r_ok, nullptr, pc, pi, nullptr, total), "capacity", "problem 0");
    expect(teaser_hip_icp_radius_search_batch(h, 2, pp, nd, qq, nq, r_ok, nullptr, pc, nullptr, nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG &&
               std::string(teaser_hip_icp_last_error(h)).find("total_out") != std::string::npos, "refusal: total_out", -1);
    expect(teaser_hip_icp_knn_search_batch(h, -1, pp, nd, qq, nq, k_ok, pi, nullptr) == TEASER_HIP_ERR_BAD_ARG, "refusal: batch", -1);
    expect(teaser_hip_icp_knn_search_batch(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_OK, "an empty batch", -1);
    expect(teaser_hip_icp_knn_search_batch(h, 2, pp, nd, qq, nq, k_ok, pi, nullptr) == TEASER_HIP_OK, "the handle works afterwards", -1);
    expect(std::vector<int32_t>(i0.begin(), i0.begin() + (size_t)cs.n_q * 5) == std::vector<int32_t>(i1.begin(), i1.begin() + (size_t)cs.n_q * 5), "two copies of a problem agree", -1);
  }
  teaser_hip_icp_destroy(h);
  std::printf("cases %d  mismatches %d\n", n_cases, g_bad);
  return g_bad ? 1 : 0;
}
