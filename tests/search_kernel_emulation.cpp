// The SOURCE of the two-cloud search kernels (csrc/kernels_search.hip: ring, hybrid, count, fill, rank) compiled for the
// host and run one thread at a time (tests/hip_stub runs a launch sequentially) against brute force, on the grids that
// csrc/icp_host.h's own set_grid / knn_edge build over the data cloud -- tests/test_search_host.py builds it with
// -fsanitize=address,undefined.  One thread at a time is exact for these kernels: a lane reads and writes only its own
// column of the LDS lists, its own outputs and (fill, rank) its own row or entry.  What is NOT emulated: the scan
// kernel of the whole-cloud route, whose merge is a wave shuffle -- a query the ring kernel puts on the worklist is only
// counted -- and the prefix kernel, whose threads talk through LDS; the exclusive sums are taken on the host here.
// With the data cloud as its own query set, the self ring kernel (csrc/kernels_outlier.hip, written out on its own) and
// the two-cloud one must give the same rows and the same worklist, query by query.
// TEST INFRASTRUCTURE ONLY.
#include <cstring>
#include <random>
#include <utility>

#include "icp_host_prelude.h"
#include "../teaser-plusplus_amd/csrc/kernels_outlier.hip"
#include "../teaser-plusplus_amd/csrc/kernels_search.hip"

using namespace thip;
typedef std::vector<double> Cloud;

static int g_fell = 0;  // worklist entries of the last run (largest list capacity)
static int g_bad_total = 0;
static void expect_fell(bool ok, const char* what) {
  if (!ok) {
    std::printf("%s: unexpected number of worklist entries (%d)\n", what, g_fell);
    ++g_bad_total;
  }
}

struct Grid {
  IcpDesc d{};
  std::vector<int32_t> bstart, qj;
  std::vector<double> qs;
};

// the index of kernels_icp.hip over the data cloud P for cell edge r (queries: n_s of them)
static void build(Grid& g, const Cloud& P, int n_s, double r) {
  const int n = (int)P.size() / 3;
  g.d = IcpDesc{};
  g.d.n_t = n, g.d.n_s = n_s, g.d.r2 = r * r;
  set_grid(g.d, P.data(), r);
  const IcpDesc& d = g.d;
  const int64_t tb = d.tb_mask + 1;
  g.bstart.assign(tb + 1, 0), g.qj.assign(n, 0), g.qs.assign(3 * n, 0.0);
  std::vector<int64_t> bk(n);
  std::vector<int32_t> cur(tb, 0);
  for (int j = 0; j < n; ++j) {
    bk[j] = icp_bucket(icp_cell(P[3 * j], d.origin[0], d.inv_h), icp_cell(P[3 * j + 1], d.origin[1], d.inv_h),
                       icp_cell(P[3 * j + 2], d.origin[2], d.inv_h), d.tb_mask);
    g.bstart[bk[j] + 1]++;
  }
  for (int64_t b = 0; b < tb; ++b) g.bstart[b + 1] += g.bstart[b];
  for (int j = n - 1; j >= 0; --j) {
    const int pos = g.bstart[bk[j]] + cur[bk[j]]++;
    g.qj[pos] = j;
    for (int c = 0; c < 3; ++c) g.qs[3 * pos + c] = P[3 * j + c];
  }
}

static std::vector<std::pair<double, int>> brute(const Cloud& P, const double* x) {
  std::vector<std::pair<double, int>> c;
  for (int j = 0; j < (int)P.size() / 3; ++j) {
    const double e0 = x[0] - P[3 * j], e1 = x[1] - P[3 * j + 1], e2 = x[2] - P[3 * j + 2];
    c.emplace_back((e0 * e0 + e1 * e1) + e2 * e2, j);
  }
  std::sort(c.begin(), c.end());
  return c;
}

template <int CAP>
static int run_ring(const Grid& g, const IcpSearchDesc& sd, const Cloud& P, const Cloud& Q, const char* name, int* fell) {
  const int n_q = (int)Q.size() / 3, k = sd.k, want = std::min(k, g.d.n_t), n_blk = (n_q + 63) / 64;
  std::vector<int32_t> blk(n_blk, 0), idx((size_t)n_q * k, -7), work(2 * n_q + 2), cnt(1, 0);
  std::vector<double> d2((size_t)n_q * k, -7.0);
  hipLaunchKernelGGL(icp_search_ring_kernel<CAP>, dim3(n_blk), dim3(64), 0, nullptr, &g.d, &sd, blk.data(), Q.data(),
                     g.qs.data(), g.qj.data(), g.bstart.data(), idx.data(), d2.data(), work.data(), cnt.data());
  std::vector<char> inwork(n_q, 0);
  for (int w = 0; w < cnt[0]; ++w) inwork[work[2 * w + 1]] = 1;
  *fell = cnt[0];
  int bad = 0;
  for (int i = 0; i < n_q; ++i) {
    if (inwork[i]) continue;
    const auto c = brute(P, &Q[3 * i]);
    for (int t = 0; t < k; ++t) {
      const int ej = t < want ? c[t].second : -1;
      const double ed = t < want ? c[t].first : INFINITY;
      if (idx[(size_t)i * k + t] != ej || d2[(size_t)i * k + t] != ed) {
        if (bad < 5) std::printf("%s ring<%d>: i %d t %d got (%g,%d) want (%g,%d)\n", name, CAP, i, t, d2[(size_t)i * k + t], idx[(size_t)i * k + t], ed, ej);
        ++bad;
      }
    }
  }
  return bad;
}

template <int CAP>
static int run_hybrid(const Grid& g, const IcpSearchDesc& sd, const Cloud& P, const Cloud& Q, const char* name) {
  const int n_q = (int)Q.size() / 3, k = sd.k, n_blk = (n_q + 63) / 64;
  std::vector<int32_t> blk(n_blk, 0), idx((size_t)n_q * k, -7), cnt(n_q, -7);
  std::vector<double> d2((size_t)n_q * k, -7.0);
  hipLaunchKernelGGL(icp_search_hybrid_kernel<CAP>, dim3(n_blk), dim3(64), 0, nullptr, &g.d, &sd, blk.data(), Q.data(),
                     g.qs.data(), g.qj.data(), g.bstart.data(), idx.data(), d2.data(), cnt.data());
  int bad = 0;
  for (int i = 0; i < n_q; ++i) {
    const auto c = brute(P, &Q[3 * i]);
    int inside = 0;
    while (inside < (int)c.size() && c[inside].first < g.d.r2) ++inside;
    const int m = std::min(k, inside);
    bool ok = cnt[i] == m;
    for (int t = 0; t < k; ++t)
      ok = ok && idx[(size_t)i * k + t] == (t < m ? c[t].second : -1) && d2[(size_t)i * k + t] == (t < m ? c[t].first : INFINITY);
    if (!ok) {
      if (bad < 5) std::printf("%s hybrid<%d>: i %d count %d want %d\n", name, CAP, i, cnt[i], m);
      ++bad;
    }
  }
  return bad;
}

static int run_radius(const Grid& g, const Cloud& P, const Cloud& Q, const char* name) {
  const int n_q = (int)Q.size() / 3, n_blk = (n_q + 255) / 256;
  std::vector<int32_t> blk(n_blk, 0), count(n_q, -7);
  hipLaunchKernelGGL(icp_search_count_kernel, dim3(n_blk), dim3(256), 0, nullptr, &g.d, blk.data(), Q.data(),
                     g.qs.data(), g.bstart.data(), count.data());
  std::vector<int64_t> prefix(n_q + 1, 0), total(2, 0);
  for (int i = 0; i < n_q; ++i) prefix[i + 1] = prefix[i] + count[i];
  const int64_t tot = prefix[n_q];
  // two problems' descriptors: the rank kernel looks its problem up; problem 0 is empty and reserves nothing
  IcpDesc ds[2] = {IcpDesc{}, g.d};
  IcpSearchDesc sds[2] = {};
  sds[0].fill = 0, sds[1].fill = 1, sds[1].capacity = tot;
  total[1] = tot;
  std::vector<int32_t> blk1(n_blk, 1), tmp_j(tot, -7), idx(tot, -7);
  std::vector<double> tmp_d2(tot, -7.0), d2(tot, -7.0);
  hipLaunchKernelGGL(icp_search_fill_kernel, dim3(n_blk), dim3(256), 0, nullptr, ds, sds, blk1.data(), Q.data(),
                     g.qs.data(), g.qj.data(), g.bstart.data(), prefix.data(), total.data(), tmp_d2.data(), tmp_j.data());
  if (tot)
    hipLaunchKernelGGL(icp_search_rank_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, nullptr, ds, sds, 2, tot,
                       count.data(), prefix.data(), total.data(), tmp_d2.data(), tmp_j.data(), idx.data(), d2.data());
  int bad = 0;
  for (int i = 0; i < n_q; ++i) {
    const auto c = brute(P, &Q[3 * i]);
    int inside = 0;
    while (inside < (int)c.size() && c[inside].first < g.d.r2) ++inside;
    bool ok = count[i] == inside;
    for (int t = 0; ok && t < inside; ++t) ok = idx[prefix[i] + t] == c[t].second && d2[prefix[i] + t] == c[t].first;
    if (!ok) {
      if (bad < 5) std::printf("%s radius: i %d count %d want %d\n", name, i, count[i], inside);
      ++bad;
    }
  }
  return bad;
}

static void run(const Cloud& P, const Cloud& Q, int k, int ring_cap, double radius, const char* name) {
  const int n = (int)P.size() / 3, n_q = (int)Q.size() / 3;
  IcpSearchDesc sd{};
  sd.k = k, sd.ring_cap = ring_cap;
  bool rings_ok = true;
  sd.edge = knn_edge(P.data(), n, std::min(k, n), &rings_ok);
  if (!rings_ok) sd.ring_cap = 0;
  Grid g;
  build(g, P, n_q, sd.edge);
  int bad = 0, fell = 0, fell_small = 0;
  bad += run_ring<kIcpKnnMax>(g, sd, P, Q, name, &fell);
  if (std::min(k, n) <= kIcpKnnSmall) {
    bad += run_ring<kIcpKnnSmall>(g, sd, P, Q, name, &fell_small);
    if (fell_small != fell) ++bad, std::printf("%s: the two capacities disagree on the worklist\n", name);
  }
  build(g, P, n_q, radius);
  bad += run_hybrid<kIcpKnnMax>(g, sd, P, Q, name);
  if (k <= kIcpKnnSmall) bad += run_hybrid<kIcpKnnSmall>(g, sd, P, Q, name);
  bad += run_radius(g, P, Q, name);
  g_fell = fell;
  g_bad_total += bad;
  std::printf("%-24s n_data %5d n_query %5d k %3d cap %2d r %-8g: fallbacks %5d  mismatches %d\n", name, n, n_q, k,
              ring_cap, radius, fell, bad);
}

// The data cloud as its own query set through the self ring kernel (icp_knn_ring_kernel: n_t queries, the
// descriptor built with n_s = 0 as the self calls build it) and through the two-cloud ring kernel
// (icp_search_ring_kernel: n_s queries): the same rows and the same worklist membership, query by query.
template <int CAP>
static int run_self_ring(const Grid& g, const IcpSearchDesc& sd, const Cloud& P, const char* name, int* fell) {
  const int n = g.d.n_t, k = sd.k, n_blk = (n + 63) / 64;
  IcpDesc self = g.d;
  self.n_s = 0;
  IcpKnnDesc kd{};
  kd.k = sd.k, kd.ring_cap = sd.ring_cap, kd.edge = sd.edge;
  std::vector<int32_t> blk(n_blk, 0);
  std::vector<int32_t> idx[2], work[2], cnt[2];
  std::vector<double> d2[2];
  for (int s = 0; s < 2; ++s) idx[s].assign((size_t)n * k, -7), d2[s].assign((size_t)n * k, -7.0), work[s].assign(2 * n + 2, 0), cnt[s].assign(1, 0);
  hipLaunchKernelGGL(icp_knn_ring_kernel<CAP>, dim3(n_blk), dim3(64), 0, nullptr, &self, &kd, blk.data(), P.data(),
                     g.qs.data(), g.qj.data(), g.bstart.data(), idx[0].data(), d2[0].data(), (double*)nullptr,
                     work[0].data(), cnt[0].data());
  hipLaunchKernelGGL(icp_search_ring_kernel<CAP>, dim3(n_blk), dim3(64), 0, nullptr, &g.d, &sd, blk.data(), P.data(),
                     g.qs.data(), g.qj.data(), g.bstart.data(), idx[1].data(), d2[1].data(), work[1].data(),
                     cnt[1].data());
  std::vector<char> inwork[2] = {std::vector<char>(n, 0), std::vector<char>(n, 0)};
  for (int s = 0; s < 2; ++s)
    for (int w = 0; w < cnt[s][0]; ++w) inwork[s][work[s][2 * w + 1]] = 1;
  *fell = cnt[0][0];
  int bad = cnt[0][0] != cnt[1][0];
  for (int i = 0; i < n; ++i) {
    bool ok = inwork[0][i] == inwork[1][i];
    for (int t = 0; t < k; ++t)  // a worklist query's row keeps its fill in both
      ok = ok && idx[0][(size_t)i * k + t] == idx[1][(size_t)i * k + t] &&
           std::memcmp(&d2[0][(size_t)i * k + t], &d2[1][(size_t)i * k + t], sizeof(double)) == 0;
    if (!ok) {
      if (bad < 5) std::printf("%s self/two-cloud ring<%d>: query %d differs (worklist %d / %d)\n", name, CAP, i, inwork[0][i], inwork[1][i]);
      ++bad;
    }
  }
  return bad;
}

static void run_self(const Cloud& P, int k, int ring_cap, const char* name) {
  const int n = (int)P.size() / 3;
  IcpSearchDesc sd{};
  sd.k = k, sd.ring_cap = ring_cap;
  bool rings_ok = true;
  sd.edge = knn_edge(P.data(), n, std::min(k, n), &rings_ok);
  if (!rings_ok) sd.ring_cap = 0;
  Grid g;
  build(g, P, n, sd.edge);
  int bad = 0, fell = 0, fell_small = 0;
  bad += run_self_ring<kIcpKnnMax>(g, sd, P, name, &fell);
  if (k <= kIcpKnnSmall) {
    bad += run_self_ring<kIcpKnnSmall>(g, sd, P, name, &fell_small);
    if (fell_small != fell) ++bad, std::printf("%s: the two capacities disagree on the worklist\n", name);
  }
  g_bad_total += bad;
  std::printf("%-24s n %5d k %3d cap %2d: self == two-cloud, fallbacks %5d  mismatches %d\n", name, n, k, sd.ring_cap,
              fell, bad);
}

int main() {
  std::mt19937_64 gen(11);
  std::uniform_real_distribution<double> u(0, 1);
  auto cube = [&](int n, double s, double off) { Cloud q(3 * n); for (double& x : q) x = u(gen) * s + off; return q; };
  auto lattice = [](int m, double h, double off) {
    Cloud q;
    for (int a = 0; a < m; ++a) for (int b = 0; b < m; ++b) for (int c = 0; c < m; ++c) { q.push_back(h * a + off); q.push_back(h * b + off); q.push_back(h * c + off); }
    return q;
  };
  // queries around the box of P for the k-NN grid of (P, k): inside, on the faces, 1 / 3 / 5 cells outside each side,
  // and 1e6 extents away
  auto around = [&](const Cloud& P, int k) {
    const int n = (int)P.size() / 3;
    bool ok = true;
    Grid g;
    build(g, P, 0, knn_edge(P.data(), n, std::min(k, n), &ok));
    const double cell = 1.0 / g.d.inv_h;
    double lo[3], hi[3], ext = 0;
    for (int c = 0; c < 3; ++c) { lo[c] = g.d.origin[c]; hi[c] = 2 * g.d.centre[c] - lo[c]; ext = std::max(ext, hi[c] - lo[c]); }
    Cloud Q;
    auto push = [&](double x, double y, double z) { Q.push_back(x); Q.push_back(y); Q.push_back(z); };
    for (int t = 0; t < 40; ++t) push(lo[0] + u(gen) * (hi[0] - lo[0]), lo[1] + u(gen) * (hi[1] - lo[1]), lo[2] + u(gen) * (hi[2] - lo[2]));
    for (int c = 0; c < 3; ++c)
      for (int side = 0; side < 2; ++side)
        for (double cells : {0.0, 0.5, 2.5, 4.5}) {  // on the face, then r0 = 1, 3, 5
          double x[3] = {g.d.centre[0], g.d.centre[1], g.d.centre[2]};
          x[c] = side ? hi[c] + cells * cell : lo[c] - cells * cell;
          push(x[0], x[1], x[2]);
          x[(c + 1) % 3] = lo[(c + 1) % 3] + 0.3 * (hi[(c + 1) % 3] - lo[(c + 1) % 3]);  // and off the axis
          push(x[0], x[1], x[2]);
        }
    push(lo[0] - 5.5 * cell, lo[1] - 5.5 * cell, hi[2] + 5.5 * cell);  // a corner, r0 = 6
    const int far_at = (int)Q.size() / 3;
    push(hi[0] + 1e6 * (ext > 0 ? ext : 1.0), g.d.centre[1], g.d.centre[2]);
    return std::make_pair(Q, far_at);
  };
  for (int k : {1, 7, 32, 33, 100})
    for (int cap : {4, 1, 0}) {
      const Cloud P = cube(1000, 1, 0);
      const auto Q = around(P, k);
      run(P, Q.first, k, cap, 0.1, "cube");
      expect_fell(cap == 0 ? g_fell == (int)Q.first.size() / 3 : g_fell >= 1, "cube: the far query goes to the worklist");
      const Cloud P2 = cube(700, 1e-3, -1e4);
      run(P2, around(P2, k).first, k, cap, 1e-4, "tiny-1e4");
    }
  {  // a dense lattice: queries at its points and at its cell centres (8-way ties) never reach the worklist
    const Cloud P = lattice(7, 0.125, 0), C = lattice(6, 0.125, 0.0625);
    for (int k : {1, 2, 8, 27, 100}) {
      run(P, P, k, 4, 0.125, "lattice points");
      expect_fell(g_fell == 0, "lattice points");
      run(P, C, k, 4, 0.125, "lattice centres");
      expect_fell(g_fell == 0, "lattice centres");
    }
    run(P, C, 8, 4, 0.25, "lattice centres r 2h");
    const auto Q = around(P, 8);
    run(P, Q.first, 8, 4, 0.125, "lattice around");
    expect_fell(g_fell >= 1, "lattice around: the far query");
  }
  {
    Cloud P = cube(500, 1, 0);
    for (int i = 0; i < 500; ++i) P[3 * i + 2] = 0.75;
    run(P, around(P, 20).first, 20, 4, 0.05, "plane");
    Cloud Q = cube(200, 1, 0);  // queries off the plane
    run(P, Q, 20, 4, 0.3, "plane, queries in the cube");
  }
  {
    Cloud P = cube(400, 1, 0);
    for (int i = 0; i < 400; ++i) { const double t = P[3 * i]; P[3 * i] = 3 + t; P[3 * i + 1] = 2 * t; P[3 * i + 2] = 1 - .5 * t; }
    run(P, around(P, 40).first, 40, 4, 0.05, "line");
  }
  {
    Cloud P(900);
    for (int i = 0; i < 300; ++i) { P[3 * i] = .3; P[3 * i + 1] = -1.25; P[3 * i + 2] = 7; }
    run(P, around(P, 5).first, 5, 4, 0.05, "same");
    run(P, cube(50, 1, 0), 100, 4, 8.0, "same100");
  }
  for (int n : {1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 513})
    for (int k : {1, 3, 100}) {
      const Cloud P = cube(n, 1, 0);
      run(P, around(P, k).first, k, 4, 0.3, "sizes");
      run(P, cube(130, 1.4, -0.2), k, 4, 2.5, "sizes, whole cloud inside r");
    }
  {
    const Cloud P = cube(5, 0.2, 0);
    for (double r : {0.05, 0.12, 0.2, 0.26, 2.0}) run(P, cube(60, 0.4, -0.1), 3, 4, r, "five");
  }
  {
    const Cloud P = cube(300, 1, 0), none;
    run(P, none, 3, 4, 0.1, "no queries");
  }
  {  // the query set is the data cloud: the self and the two-cloud ring kernel, bit for bit
    std::vector<std::pair<Cloud, const char*>> clouds;
    clouds.emplace_back(cube(1000, 1, 0), "self: cube");
    clouds.emplace_back(lattice(7, 0.125, 0), "self: lattice");
    Cloud far = cube(300, 1, 0);  // two far outliers: they are the ones that may reach the worklist
    far[3 * 17] = 1e3, far[3 * 211 + 1] = 1e6;
    clouds.emplace_back(far, "self: two far outliers");
    for (int n : {1, 2, 63, 64, 65, 257}) clouds.emplace_back(cube(n, 1, 0), "self: sizes");
    for (const auto& c : clouds)
      for (int k : {1, 32, 33, 100})
        for (int cap : {4, 1}) run_self(c.first, k, cap, c.second);
  }
  std::printf("TOTAL mismatches %d\n", g_bad_total);
  return g_bad_total != 0;
}
