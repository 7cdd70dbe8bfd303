// The SOURCE of the ring-search and radius-count kernels (csrc/kernels_outlier.hip) compiled for the host and run one
// thread at a time (tests/hip_stub runs a launch sequentially) against brute force, with the grids that csrc/icp_host.h's
// own set_grid / knn_edge build (the handle's host files are part of this translation unit) -- tests/test_outlier_host.py builds it
// with -fsanitize=address,undefined.  One lane at a time is exact for these two kernels: a lane reads and writes only
// its own column of the LDS lists and its own outputs.  The wave-wide operations are NOT emulated: the kept counts (a
// ballot) are not compared, and a query the ring kernel puts on the worklist is only counted -- the scan kernel, whose
// merge is a wave shuffle, does not run here.
// TEST INFRASTRUCTURE ONLY.
#include <random>

#include "icp_host_prelude.h"
#include "../teaser-plusplus_amd/csrc/kernels_outlier.hip"
#include "../teaser-plusplus_amd/csrc/icp.hip"
#include "../teaser-plusplus_amd/csrc/icp_outlier.hip"

static int g_fell = 0;  // worklist entries of the last run
static int expect_fell(bool ok, const char* what) {
  if (!ok) std::printf("%s: unexpected number of worklist entries (%d)\n", what, g_fell);
  return ok ? 0 : 1;
}

static int run(const std::vector<double>& q, int k, int ring_cap, double radius, const char* name) {
  const int n = (int)q.size() / 3;
  IcpDesc d{}; IcpKnnDesc kd{};
  d.n_t = n; kd.k = k; kd.ring_cap = ring_cap;
  const int want = std::min(k, n);
  int bad = 0, fell = 0;
  for (int mode = 0; mode < 2; ++mode) {  // 0: knn grid, 1: radius grid
    bool rings_ok = true;
    kd.edge = mode ? radius : knn_edge(q.data(), n, want, &rings_ok);
    d.r2 = kd.edge * kd.edge;
    set_grid(d, q.data(), kd.edge);
    const int64_t tb = d.tb_mask + 1;
    std::vector<int32_t> bstart(tb + 1, 0), qj(n), cur(tb, 0);
    std::vector<double> qs(3 * n);
    std::vector<int64_t> bk(n);
    for (int j = 0; j < n; ++j) { bk[j] = icp_bucket(icp_cell(q[3*j], d.origin[0], d.inv_h), icp_cell(q[3*j+1], d.origin[1], d.inv_h), icp_cell(q[3*j+2], d.origin[2], d.inv_h), d.tb_mask); bstart[bk[j] + 1]++; }
    for (int64_t b = 0; b < tb; ++b) bstart[b + 1] += bstart[b];
    for (int j = n - 1; j >= 0; --j) { const int pos = bstart[bk[j]] + cur[bk[j]]++; qj[pos] = j; for (int c = 0; c < 3; ++c) qs[3*pos+c] = q[3*j+c]; }
    const int n_blk = (n + 63) / 64, n_tblk = (n + 255) / 256;
    std::vector<int32_t> blk(n_blk, 0), tblk(n_tblk, 0);
    if (mode == 0) {
      std::vector<int32_t> idx((size_t)n * k, -7), work(2 * n), cnt(1, 0);
      std::vector<double> d2((size_t)n * k, -7.0);
      hipLaunchKernelGGL(icp_knn_ring_kernel<kIcpKnnMax>, dim3(n_blk), dim3(64), 0, nullptr, &d, &kd, blk.data(), q.data(), qs.data(), qj.data(), bstart.data(), idx.data(), d2.data(), (double*)nullptr, work.data(), cnt.data());
      std::vector<char> inwork(n, 0);
      for (int w = 0; w < cnt[0]; ++w) inwork[work[2*w+1]] = 1;
      fell = cnt[0];
      for (int i = 0; i < n; ++i) {
        if (inwork[i]) continue;
        std::vector<std::pair<double,int>> c;
        for (int j = 0; j < n; ++j) { const double e0=q[3*i]-q[3*j], e1=q[3*i+1]-q[3*j+1], e2=q[3*i+2]-q[3*j+2]; c.emplace_back((e0*e0+e1*e1)+e2*e2, j); }
        std::sort(c.begin(), c.end());
        for (int t = 0; t < k; ++t) {
          const int ej = t < want ? c[t].second : -1; const double ed = t < want ? c[t].first : INFINITY;
          if (idx[(size_t)i*k+t] != ej || d2[(size_t)i*k+t] != ed) { if (bad < 5) std::printf("%s: i %d t %d got (%g,%d) want (%g,%d)\n", name, i, t, d2[(size_t)i*k+t], idx[(size_t)i*k+t], ed, ej); ++bad; }
        }
      }
    } else {
      std::vector<int32_t> count(n, -1), kept(1, 0); std::vector<uint8_t> keep(n, 9);
      kd.k = 2;
      hipLaunchKernelGGL(icp_radius_count_kernel, dim3(n_tblk), dim3(256), 0, nullptr, &d, &kd, tblk.data(), q.data(), qs.data(), bstart.data(), count.data(), keep.data(), kept.data());
      for (int i = 0; i < n; ++i) {
        int c = 0;
        for (int j = 0; j < n; ++j) { const double e0=q[3*i]-q[3*j], e1=q[3*i+1]-q[3*j+1], e2=q[3*i+2]-q[3*j+2]; c += (e0*e0+e1*e1)+e2*e2 < d.r2; }
        if (count[i] != c || keep[i] != (c > 2)) { if (bad < 5) std::printf("%s radius: i %d got %d want %d\n", name, i, count[i], c); ++bad; }
      }
    }
  }
  g_fell = fell;
  std::printf("%-28s n %5d k %3d cap %2d: fallbacks %5d  mismatches %d\n", name, n, k, ring_cap, fell, bad);
  return bad;
}

int main() {
  std::mt19937_64 g(7);
  std::uniform_real_distribution<double> u(0, 1);
  auto cube = [&](int n, double s, double off) { std::vector<double> q(3 * n); for (double& x : q) x = u(g) * s + off; return q; };
  int bad = 0;
  for (int k : {1, 7, 20, 100}) for (int cap : {4, 1}) {
    bad += run(cube(1000, 1, 0), k, cap, 0.1, "cube");
    bad += run(cube(1000, 1, 1e4), k, cap, 0.1, "cube+1e4");
    bad += run(cube(1000, 1e-3, -1e4), k, cap, 1e-4, "tiny-1e4");
  }
  { std::vector<double> q; for (int a=0;a<7;++a) for (int b=0;b<7;++b) for (int c=0;c<7;++c) { q.push_back(.125*a); q.push_back(.125*b); q.push_back(.125*c);} for (int k : {1,2,7,27,100}) bad += run(q, k, 4, 0.125, "lattice"); bad += run(q, 27, 16, 0.25, "lattice16"); }
  { auto q = cube(2002, 1, 0); for (int c=0;c<3;++c){ q[3*700+c]=1000; q[3*1300+c]=1e6;} bad += run(q, 20, 4, 0.1, "far"); bad += expect_fell(g_fell >= 1 && g_fell < 2002, "far"); bad += run(q, 100, 4, 0.1, "far100"); bad += run(q, 1, 4, 0.1, "far1"); }
  { auto q = cube(500, 1, 0); for (int i=0;i<500;++i) q[3*i+2]=0.75; bad += run(q, 20, 4, 0.05, "plane"); bad += expect_fell(g_fell == 0, "plane"); bad += run(q, 20, 16, 0.05, "plane16"); }
  { auto q = cube(400, 1, 0); for (int i=0;i<400;++i){ double t=q[3*i]; q[3*i]=3+t; q[3*i+1]=2*t; q[3*i+2]=1-.5*t;} bad += run(q, 40, 4, 0.05, "line"); bad += expect_fell(g_fell == 0, "line"); }
  { std::vector<double> q(900); for (int i=0;i<300;++i){q[3*i]=.3;q[3*i+1]=-1.25;q[3*i+2]=7;} bad += run(q, 5, 4, 0.05, "same"); bad += run(q, 100, 4, 0.05, "same100"); }
  for (int n : {1,2,3,5,255,256,257,513}) for (int k : {1,3,100}) bad += run(cube(n,1,0), k, 4, 0.3, "sizes");
  { auto q = cube(500,1,0); for (int i=1;i<40;++i) for(int c=0;c<3;++c) q[3*(i*7)+c]=q[c]; bad += run(q, 20, 4, 0.1, "dups"); }
  { auto q = cube(5,0.2,0); for (double r : {0.05,0.12,0.2,0.26,2.0}) bad += run(q, 3, 4, r, "five"); }
  { auto q = cube(400,1,0); for (int i=0;i<400;++i){ q[3*i+1]*=1e-170; q[3*i+2]*=1e-171;} bad += run(q, 20, 4, 0.05, "nearline"); bad += expect_fell(g_fell == 0, "nearline"); }
  std::printf("TOTAL mismatches %d\n", bad);
  return bad != 0;
}
