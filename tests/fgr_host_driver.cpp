// Host-only check of csrc/fgr.hip (tests/test_fgr_host.py): compiled by g++ against the HIP stand-in header
// (tests/hip_stub) with -fsanitize=address,undefined as a stand-alone program.  The launchers are stand-ins that run the
// one-lane functions of csrc/fgr_device.h on the CPU, one lane at a time, into the very buffers the host side sized and
// packed (a wrong size or offset is an AddressSanitizer report or a wrong value): the normalisation with its block
// partials, the resident route as one call per problem, the streamed route launch by launch through the partials
// buffer.  Checked: the packing and the offsets of mixed batches; the route of every problem at resident_max_corr 0,
// the default and the bound; the full call and the stage call against the contract written out here; the stage call's
// layout with NULL outputs; every refusal with its argument and problem.
//   fgr_host_driver    exit code 0 and "mismatches 0": every expectation met
// TEST INFRASTRUCTURE ONLY.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <limits>

#include "../teaser-plusplus_amd/csrc/fgr.hip"

thread_local stub_dim3_ blockIdx, threadIdx, gridDim, blockDim;

static int g_bad = 0;
#define EXPECT(c)                                                \
  do {                                                           \
    if (!(c)) {                                                  \
      ++g_bad;                                                   \
      printf("line %d: expectation failed: %s\n", __LINE__, #c); \
    }                                                            \
  } while (0)

static int g_normalise = 0, g_resident = 0, g_steps = 0, g_moves = 0, g_finishes = 0, g_last_res_blk = 0;
static std::vector<int> g_res_problems, g_str_problems;

// ---- the block order, one lane at a time ----
static double block256(const double* v) {
  double w[4];
  for (int wave = 0; wave < 4; ++wave) {
    double a[64], t[64];
    for (int l = 0; l < 64; ++l) a[l] = v[64 * wave + l];
    for (int o = 32; o > 0; o >>= 1) {
      for (int l = 0; l < 64; ++l) t[l] = a[l] + a[l ^ o];
      for (int l = 0; l < 64; ++l) a[l] = t[l];
    }
    w[wave] = a[0];
  }
  return (w[0] + w[1]) + (w[2] + w[3]);
}

// partials of nblk blocks, `stride` doubles apart -> the sum
static double combine(const double* part, int nblk, int stride) {
  double acc[256];
  for (int t = 0; t < 256; ++t) {
    acc[t] = 0.0;
    for (int b = t; b < nblk; b += 256) acc[t] += part[(int64_t)b * stride];
  }
  return block256(acc);
}

namespace thip {

void launch_fgr_normalise(hipStream_t, int batch, int max_cloud_blk, int max_pair_blk, const FgrBufs& B) {
  ++g_normalise;
  int seen_cloud = 0, seen_pair = 0;
  for (int p = 0; p < batch; ++p) {
    const FgrDesc& D = B.desc[p];
    FgrState& st = B.state[p];
    double mx = 0.0;
    for (int side = 0; side < 2; ++side) {
      const int n = side ? D.n_t : D.n_s;
      const double* X = side ? B.dst + 3 * D.dst_off : B.src + 3 * D.src_off;
      const int64_t off = side ? D.tblk_off : D.sblk_off;
      const int nblk = (n + 255) / 256;
      seen_cloud = std::max(seen_cloud, nblk);
      for (int b = 0; b < nblk; ++b)
        for (int k = 0; k < 3; ++k) {
          double v[256];
          for (int l = 0; l < 256; ++l) v[l] = 256 * b + l < n ? X[3 * (256 * (int64_t)b + l) + k] : 0.0;
          B.cloud_sum[3 * (off + b) + k] = block256(v);
        }
      for (int k = 0; k < 3; ++k) st.mean[3 * side + k] = combine(B.cloud_sum + 3 * off + k, nblk, 3) / (double)n;
      for (int b = 0; b < nblk; ++b) {
        double m = 0.0;
        for (int l = 0; l < 256 && 256 * b + l < n; ++l) m = fmax(m, fgr_norm(X + 3 * (256 * (int64_t)b + l), st.mean + 3 * side));
        B.cloud_max[off + b] = m;
        mx = fmax(mx, m);
      }
    }
    fgr_start(D, st, mx);
    seen_pair = std::max(seen_pair, (D.ncorr + 255) / 256);
    for (int c = 0; c < D.ncorr; ++c) {
      const int64_t i = B.corr[2 * (D.corr_off + c)], j = B.corr[2 * (D.corr_off + c) + 1];
      fgr_record(st, B.src + 3 * (D.src_off + i), B.dst + 3 * (D.dst_off + j), B.pairs + 6 * (D.corr_off + c));
    }
  }
  EXPECT(seen_cloud == max_cloud_blk);
  EXPECT(seen_pair == max_pair_blk);
}

// the 27 sums of problem p at its current records; part: room for its block partials
static void sums(const FgrBufs& B, int p, double* part, double* tot) {
  const FgrDesc& D = B.desc[p];
  const int nblk = (D.ncorr + 255) / 256;
  for (int b = 0; b < nblk; ++b) {
    static double v[FGR_SUMS][256];
    for (int l = 0; l < 256; ++l) {
      double t[FGR_SUMS];
      for (int k = 0; k < FGR_SUMS; ++k) t[k] = 0.0;
      const int c = 256 * b + l;
      if (c < D.ncorr) fgr_terms(B.pairs + 6 * (D.corr_off + c), B.pairs + 6 * (D.corr_off + c) + 3, B.state[p].mu, t);
      for (int k = 0; k < FGR_SUMS; ++k) v[k][l] = t[k];
    }
    for (int k = 0; k < FGR_SUMS; ++k) part[(int64_t)b * FGR_SUMS + k] = block256(v[k]);
  }
  for (int k = 0; k < FGR_SUMS; ++k) tot[k] = combine(part + k, nblk, FGR_SUMS);
}

static void move(const FgrBufs& B, int p) {
  const FgrDesc& D = B.desc[p];
  for (int c = 0; c < D.ncorr; ++c) fgr_apply(B.state[p].delta, B.pairs + 6 * (D.corr_off + c) + 3);
}

hipError_t launch_fgr_resident(hipStream_t, int n, const int32_t* idx, int max_blk, const FgrBufs& B, int keep) {
  if (n <= 0) return hipSuccess;
  ++g_resident;
  g_last_res_blk = max_blk;
  EXPECT(max_blk >= 1 && max_blk <= FGR_RES_MAX_BLK);
  for (int q = 0; q < n; ++q) {
    const int p = idx[q];
    g_res_problems.push_back(p);
    const FgrDesc& D = B.desc[p];
    EXPECT(D.run && (D.ncorr + 255) / 256 <= max_blk);
    if (!fgr_live(D, B.state[p])) continue;
    std::vector<double> part((size_t)max_blk * FGR_SUMS), saved;
    if (!keep) saved.assign(B.pairs + 6 * D.corr_off, B.pairs + 6 * (D.corr_off + D.ncorr));
    for (int itr = 0; itr < D.n_iter; ++itr) {
      double tot[FGR_SUMS];
      sums(B, p, part.data(), tot);
      fgr_step(D, B.state[p], tot, B.log ? B.log + (int64_t)p * B.log_stride : nullptr);
      move(B, p);
    }
    if (!keep) std::copy(saved.begin(), saved.end(), B.pairs + 6 * D.corr_off);  // the records stay in LDS on the device
  }
  return hipSuccess;
}

void launch_fgr_streamed_step(hipStream_t, int n, const int32_t* idx, int max_blk, const FgrBufs& B, int itr) {
  if (n <= 0 || max_blk <= 0) return;
  ++g_steps;
  for (int q = 0; q < n; ++q) {
    const int p = idx[q];
    if (itr == 0) g_str_problems.push_back(p);
    const FgrDesc& D = B.desc[p];
    EXPECT(D.run && (D.ncorr + 255) / 256 <= max_blk);
    if (itr >= D.n_iter || !fgr_live(D, B.state[p])) continue;
    if (itr > 0) move(B, p);
    double tot[FGR_SUMS];
    sums(B, p, B.partials + D.pblk_off * FGR_SUMS, tot);
    fgr_step(D, B.state[p], tot, B.log ? B.log + (int64_t)p * B.log_stride : nullptr);
  }
}

void launch_fgr_streamed_move(hipStream_t, int n, const int32_t* idx, int max_blk, const FgrBufs& B) {
  if (n <= 0 || max_blk <= 0) return;
  ++g_moves;
  for (int q = 0; q < n; ++q) {
    const FgrDesc& D = B.desc[idx[q]];
    if (D.n_iter > 0 && fgr_live(D, B.state[idx[q]])) move(B, idx[q]);
  }
}

void launch_fgr_finish(hipStream_t, int batch, const FgrBufs& B) {
  ++g_finishes;
  for (int p = 0; p < batch; ++p) fgr_finish(B.state[p]);
}

}  // namespace thip

// ---- problems ----
struct Problem {
  std::vector<double> P, Q;
  std::vector<int32_t> corr;
  teaser_fgr_params_c prm;
};

static uint64_t g_rng = 12345;
static double uni() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_rng >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

static Problem make_problem(int ns, int nt, int ncorr, int iterations) {
  Problem p;
  for (int k = 0; k < 3 * ns; ++k) p.P.push_back(uni());
  for (int k = 0; k < 3 * nt; ++k) p.Q.push_back(uni());
  const double c = cos(0.4), sn = sin(0.4);
  for (int k = 0; k < ncorr; ++k) {
    const int i = (7 * k + 1) % ns, j = (13 * k + 2) % nt;
    p.corr.push_back(i);
    p.corr.push_back(j);
    if (k % 3 != 0) {
      const double* a = &p.P[3 * i];
      p.Q[3 * j] = c * a[0] - sn * a[1] + 0.3 + 1e-3 * uni();
      p.Q[3 * j + 1] = sn * a[0] + c * a[1] - 0.2 + 1e-3 * uni();
      p.Q[3 * j + 2] = a[2] + 0.1 + 1e-3 * uni();
    }
  }
  teaser_hip_fgr_params_default(&p.prm);
  p.prm.iteration_number = iterations;
  return p;
}

struct Expected {
  teaser_fgr_result_c r;
  std::vector<FgrLog> log;
  std::vector<double> p, q;
};

// The contract, written out for one problem alone (n < 0: the full call).
static Expected expected(const Problem& pr, int n) {
  Expected e;
  const int ns = (int)pr.P.size() / 3, nt = (int)pr.Q.size() / 3, nc = (int)pr.corr.size() / 2;
  FgrDesc D;
  memset(&D, 0, sizeof(D));
  D.div = pr.prm.division_factor;
  D.maxd = pr.prm.maximum_correspondence_distance;
  D.n_s = ns;
  D.n_t = nt;
  D.ncorr = nc;
  D.n_iter = n < 0 ? pr.prm.iteration_number : n;
  D.abs_scale = pr.prm.use_absolute_scale;
  D.decrease_mu = pr.prm.decrease_mu;
  D.run = nc >= 10;
  FgrState st;
  memset(&st, 0, sizeof(st));
  double mx = 0.0;
  for (int side = 0; side < 2; ++side) {
    const std::vector<double>& X = side ? pr.Q : pr.P;
    const int m = side ? nt : ns, nblk = (m + 255) / 256;
    for (int k = 0; k < 3; ++k) {
      std::vector<double> part((size_t)nblk);
      for (int b = 0; b < nblk; ++b) {
        double v[256];
        for (int l = 0; l < 256; ++l) v[l] = 256 * b + l < m ? X[3 * (256 * (size_t)b + l) + k] : 0.0;
        part[(size_t)b] = block256(v);
      }
      st.mean[3 * side + k] = combine(part.data(), nblk, 1) / (double)m;
    }
    for (int i = 0; i < m; ++i) mx = fmax(mx, fgr_norm(&X[3 * (size_t)i], st.mean + 3 * side));
  }
  fgr_start(D, st, mx);
  e.p.resize(3 * (size_t)nc);
  e.q.resize(3 * (size_t)nc);
  for (int c = 0; c < nc; ++c) {
    double rec[6];
    fgr_record(st, &pr.P[3 * (size_t)pr.corr[2 * c]], &pr.Q[3 * (size_t)pr.corr[2 * c + 1]], rec);
    for (int k = 0; k < 3; ++k) e.p[3 * c + k] = rec[k], e.q[3 * c + k] = rec[3 + k];
  }
  e.log.resize((size_t)std::max(D.n_iter, 1));
  memset(e.log.data(), 0, sizeof(FgrLog) * e.log.size());
  const int nblk = (nc + 255) / 256;
  for (int itr = 0; itr < D.n_iter && fgr_live(D, st); ++itr) {
    double tot[FGR_SUMS];
    for (int k = 0; k < FGR_SUMS; ++k) {
      std::vector<double> part((size_t)nblk);
      for (int b = 0; b < nblk; ++b) {
        double v[256];
        for (int l = 0; l < 256; ++l) {
          double t[FGR_SUMS];
          for (int z = 0; z < FGR_SUMS; ++z) t[z] = 0.0;
          const int c = 256 * b + l;
          if (c < nc) fgr_terms(&e.p[3 * (size_t)c], &e.q[3 * (size_t)c], st.mu, t);
          v[l] = t[k];
        }
        part[(size_t)b] = block256(v);
      }
      tot[k] = combine(part.data(), nblk, 1);
    }
    fgr_step(D, st, tot, e.log.data());
    for (int c = 0; c < nc; ++c) fgr_apply(st.delta, &e.q[3 * (size_t)c]);
  }
  fgr_finish(st);
  memset(&e.r, 0, sizeof(e.r));
  memcpy(e.r.transformation, st.T, sizeof(st.T));
  memcpy(e.r.optimised, st.trans, sizeof(st.trans));
  e.r.scale_global = st.scale_global;
  e.r.scale_start = st.scale_start;
  e.r.final_mu = st.mu;
  e.r.iterations = st.iterations;
  e.r.n_corr = nc;
  e.r.failed_solves = st.failed;
  e.r.flags = st.flags;
  return e;
}

struct Batch {
  std::vector<const double*> src, dst;
  std::vector<const int32_t*> corr;
  std::vector<int32_t> ns, nt, nc;
  std::vector<teaser_fgr_params_c> prm;
  explicit Batch(const std::vector<Problem>& ps) {
    for (const Problem& p : ps) {
      src.push_back(p.P.data());
      dst.push_back(p.Q.data());
      corr.push_back(p.corr.empty() ? nullptr : p.corr.data());
      ns.push_back((int32_t)p.P.size() / 3);
      nt.push_back((int32_t)p.Q.size() / 3);
      nc.push_back((int32_t)p.corr.size() / 2);
      prm.push_back(p.prm);
    }
  }
};

static bool same(const teaser_fgr_result_c& a, const teaser_fgr_result_c& b) { return memcmp(&a, &b, sizeof(a)) == 0; }

static void expect_refusal(teaser_hip_fgr* h, int32_t rc, const char* what, int problem) {
  const std::string msg = teaser_hip_fgr_last_error(h);
  const bool ok = rc == TEASER_HIP_ERR_BAD_ARG && msg.find(what) != std::string::npos &&
                  (problem < 0 || msg.find("(problem " + std::to_string(problem) + ")") != std::string::npos);
  if (!ok) {
    ++g_bad;
    printf("refusal '%s' (problem %d): got status %d, '%s'\n", what, problem, rc, msg.c_str());
  }
}

int main() {
  teaser_hip_fgr* h = nullptr;
  EXPECT(teaser_hip_fgr_create(-1, &h) == TEASER_HIP_OK && h);
  int64_t v = -1;
  EXPECT(teaser_hip_fgr_get_option(h, "resident_max_corr", &v) == TEASER_HIP_OK && v == 256);
  EXPECT(fgr_route(9, 1024) == 0 && fgr_route(10, 1024) == 1 && fgr_route(1024, 1024) == 1 && fgr_route(1025, 1024) == 2);
  EXPECT(fgr_route(10, 0) == 2 && fgr_route(3072, 3072) == 1 && fgr_route(3073, 3072) == 2);

  // a mixed batch: not optimised, resident at every setting but 0, resident only above the default, streamed always
  std::vector<Problem> ps;
  ps.push_back(make_problem(40, 57, 9, 64));
  ps.push_back(make_problem(300, 257, 65, 64));
  ps.push_back(make_problem(700, 513, 1025, 5));
  ps.push_back(make_problem(256, 1500, 3073, 3));
  ps.push_back(make_problem(33, 21, 10, 0));
  ps[1].prm.use_absolute_scale = 1;
  ps[2].prm.decrease_mu = 0;
  ps[3].prm.maximum_correspondence_distance = 0.6;
  Problem same_point = make_problem(12, 12, 12, 4);  // scale 0: every point the same, the mean exact
  for (double& x : same_point.P) x = 0.5;
  for (double& x : same_point.Q) x = -1.25;
  ps.push_back(same_point);
  const int B = (int)ps.size();
  std::vector<Expected> want;
  for (const Problem& p : ps) want.push_back(expected(p, -1));
  EXPECT(want[0].r.flags == 1 && want[0].r.iterations == 0 && want[5].r.flags == 2 && want[5].r.iterations == 0);
  EXPECT(want[1].r.iterations == 64 && want[1].r.failed_solves == 0 && want[4].r.iterations == 0 && want[4].r.flags == 0);
  EXPECT(want[5].r.transformation[3] == -1.75 && want[0].r.optimised[0] == 1.0);
  Batch bt(ps);
  const struct { int64_t knob; std::vector<int> res, str; } routes[] = {
      {0, {}, {1, 2, 3, 4, 5}}, {256, {1, 4, 5}, {2, 3}}, {3072, {1, 2, 4, 5}, {3}}};
  for (const auto& rt : routes) {
    EXPECT(teaser_hip_fgr_set_option(h, "resident_max_corr", rt.knob) == TEASER_HIP_OK);
    g_res_problems.clear();
    g_str_problems.clear();
    const int steps0 = g_steps, fin0 = g_finishes, norm0 = g_normalise, moves0 = g_moves;
    std::vector<teaser_fgr_result_c> out((size_t)B);
    const int32_t rc = teaser_hip_fgr_correspondence_batch(h, B, bt.src.data(), bt.ns.data(), bt.dst.data(), bt.nt.data(),
                                                           bt.corr.data(), bt.nc.data(), bt.prm.data(), out.data());
    EXPECT(rc == TEASER_HIP_OK);
    EXPECT(g_res_problems == rt.res && g_str_problems == rt.str);
    EXPECT(g_finishes == fin0 + 1 && g_normalise == norm0 + 1 && g_moves == moves0);
    int max_iter = 0;
    for (int p : rt.str) max_iter = std::max(max_iter, (int)ps[(size_t)p].prm.iteration_number);
    EXPECT(g_steps == steps0 + max_iter);  // one streamed launch pair an iteration, as many as the longest problem asks
    if (rt.knob == 3072) EXPECT(g_last_res_blk == 5);
    for (int b = 0; b < B; ++b) EXPECT(same(out[(size_t)b], want[(size_t)b].r));
    // every problem alone
    for (int b = 0; b < B; ++b) {
      teaser_fgr_result_c one;
      EXPECT(teaser_hip_fgr_correspondence(h, bt.src[b], bt.ns[b], bt.dst[b], bt.nt[b], bt.corr[b], bt.nc[b], &bt.prm[b],
                                           &one) == TEASER_HIP_OK);
      EXPECT(same(one, want[(size_t)b].r));
    }
  }

  // the stage call: n = 3 on the problems that allow it, both routes, every output and none
  {
    std::vector<Problem> qs = {ps[1], ps[0], ps[3], ps[2]};
    Batch sb(qs);
    const int n = 3, SB = (int)qs.size();
    std::vector<Expected> sw;
    int64_t total = 0;
    for (const Problem& p : qs) {
      sw.push_back(expected(p, n));
      total += (int64_t)p.corr.size() / 2;
    }
    for (int64_t knob : {(int64_t)0, (int64_t)256, (int64_t)3072}) {
      EXPECT(teaser_hip_fgr_set_option(h, "resident_max_corr", knob) == TEASER_HIP_OK);
      std::vector<teaser_fgr_result_c> out((size_t)SB);
      std::vector<double> mu((size_t)SB * n, -1), A((size_t)SB * n * 36, -1), g((size_t)SB * n * 6, -1),
          xi((size_t)SB * n * 6, -1), tr((size_t)SB * n * 16, -1), pp((size_t)total * 3, -1), qq((size_t)total * 3, -1);
      std::vector<int32_t> fl((size_t)SB * n, -1);
      const int moves0 = g_moves;
      EXPECT(teaser_hip_fgr_iterations_batch(h, SB, sb.src.data(), sb.ns.data(), sb.dst.data(), sb.nt.data(),
                                             sb.corr.data(), sb.nc.data(), sb.prm.data(), n, out.data(), mu.data(),
                                             A.data(), g.data(), xi.data(), fl.data(), tr.data(), pp.data(),
                                             qq.data()) == TEASER_HIP_OK);
      EXPECT(g_moves == moves0 + 1);
      int64_t first = 0;
      for (int b = 0; b < SB; ++b) {
        const Expected& e = sw[(size_t)b];
        EXPECT(same(out[(size_t)b], e.r));
        for (int k = 0; k < n; ++k) {
          const FgrLog& L = e.log[(size_t)k];
          const size_t at = (size_t)b * n + k;
          EXPECT(mu[at] == L.mu && fl[at] == L.flag);
          EXPECT(memcmp(&A[36 * at], L.A, sizeof(L.A)) == 0 && memcmp(&g[6 * at], L.g, sizeof(L.g)) == 0);
          EXPECT(memcmp(&xi[6 * at], L.xi, sizeof(L.xi)) == 0 && memcmp(&tr[16 * at], L.trans, sizeof(L.trans)) == 0);
        }
        const size_t m = e.p.size();
        EXPECT(m == 0 || (memcmp(&pp[3 * (size_t)first], e.p.data(), sizeof(double) * m) == 0 &&
                          memcmp(&qq[3 * (size_t)first], e.q.data(), sizeof(double) * m) == 0));
        first += (int64_t)m / 3;
      }
      EXPECT(sw[0].log[0].mu > 0 && sw[0].log[2].A[21] > 0 && sw[1].log[0].mu == 0);  // the 9-pair problem leaves zeros
      // every output NULL
      EXPECT(teaser_hip_fgr_iterations_batch(h, SB, sb.src.data(), sb.ns.data(), sb.dst.data(), sb.nt.data(),
                                             sb.corr.data(), sb.nc.data(), sb.prm.data(), n, nullptr, nullptr, nullptr,
                                             nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_OK);
      // n = 0: the records before any step
      std::vector<double> p0((size_t)total * 3, -1), q0((size_t)total * 3, -1);
      EXPECT(teaser_hip_fgr_iterations_batch(h, SB, sb.src.data(), sb.ns.data(), sb.dst.data(), sb.nt.data(),
                                             sb.corr.data(), sb.nc.data(), sb.prm.data(), 0, out.data(), nullptr, nullptr,
                                             nullptr, nullptr, nullptr, nullptr, p0.data(), q0.data()) == TEASER_HIP_OK);
      const Expected e0 = expected(qs[0], 0);
      EXPECT(memcmp(p0.data(), e0.p.data(), sizeof(double) * e0.p.size()) == 0 &&
             memcmp(q0.data(), e0.q.data(), sizeof(double) * e0.q.size()) == 0 && same(out[0], e0.r));
      EXPECT(memcmp(p0.data(), pp.data(), sizeof(double) * e0.p.size()) == 0);
    }
    // n above a problem's iteration_number (problem 2 has 3, problem 3 has 5)
    expect_refusal(h, teaser_hip_fgr_iterations_batch(h, SB, sb.src.data(), sb.ns.data(), sb.dst.data(), sb.nt.data(),
                                                      sb.corr.data(), sb.nc.data(), sb.prm.data(), 4, nullptr, nullptr,
                                                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
                   "n must be in 0 .. iteration_number", 2);
    expect_refusal(h, teaser_hip_fgr_iterations_batch(h, SB, sb.src.data(), sb.ns.data(), sb.dst.data(), sb.nt.data(),
                                                      sb.corr.data(), sb.nc.data(), sb.prm.data(), -1, nullptr, nullptr,
                                                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
                   "n must be in 0 .. iteration_number", -1);
  }

  // ---- every refusal, with nothing launched ----
  {
    const int norm0 = g_normalise;
    std::vector<teaser_fgr_result_c> out((size_t)B);
    auto call = [&](Batch& b) {
      return teaser_hip_fgr_correspondence_batch(h, B, b.src.data(), b.ns.data(), b.dst.data(), b.nt.data(),
                                                 b.corr.data(), b.nc.data(), b.prm.data(), out.data());
    };
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    { Batch b(ps); b.prm[2].division_factor = 1.0; expect_refusal(h, call(b), "division_factor", 2); }
    { Batch b(ps); b.prm[1].division_factor = nan; expect_refusal(h, call(b), "division_factor", 1); }
    { Batch b(ps); b.prm[3].maximum_correspondence_distance = 0; expect_refusal(h, call(b), "maximum_correspondence_distance", 3); }
    { Batch b(ps); b.prm[3].maximum_correspondence_distance = inf; expect_refusal(h, call(b), "maximum_correspondence_distance", 3); }
    { Batch b(ps); b.prm[0].iteration_number = -1; expect_refusal(h, call(b), "iteration_number", 0); }
    { Batch b(ps); b.prm[4].iteration_number = 1025; expect_refusal(h, call(b), "iteration_number", 4); }
    { Batch b(ps); b.prm[1].use_absolute_scale = 2; expect_refusal(h, call(b), "use_absolute_scale", 1); }
    { Batch b(ps); b.prm[1].decrease_mu = -1; expect_refusal(h, call(b), "decrease_mu", 1); }
    { Batch b(ps); b.ns[2] = 0; expect_refusal(h, call(b), "source is empty", 2); }
    { Batch b(ps); b.nt[5] = 0; expect_refusal(h, call(b), "target is empty", 5); }
    { Batch b(ps); b.nc[1] = -1; expect_refusal(h, call(b), "n_corr", 1); }
    { Batch b(ps); b.src[3] = nullptr; expect_refusal(h, call(b), "src is NULL", 3); }
    { Batch b(ps); b.dst[0] = nullptr; expect_refusal(h, call(b), "dst is NULL", 0); }
    { Batch b(ps); b.corr[2] = nullptr; expect_refusal(h, call(b), "corr is NULL", 2); }
    { std::vector<Problem> q = ps; q[1].P[5] = nan; Batch b(q); expect_refusal(h, call(b), "src has non-finite", 1); }
    { std::vector<Problem> q = ps; q[4].Q[0] = inf; Batch b(q); expect_refusal(h, call(b), "dst has non-finite", 4); }
    { std::vector<Problem> q = ps; q[2].corr[8] = 700; Batch b(q); expect_refusal(h, call(b), "source index of pair 4", 2); }
    { std::vector<Problem> q = ps; q[3].corr[7] = -1; Batch b(q); expect_refusal(h, call(b), "target index of pair 3", 3); }
    { std::vector<Problem> q = ps; q[1].corr[8] = 300; Batch b(q); expect_refusal(h, call(b), "source index of pair 4", 1); }
    EXPECT(std::string(teaser_hip_fgr_last_error(h)) == "corr: source index of pair 4 is outside the cloud (problem 1)");
    { std::vector<Problem> q = ps; q[1].corr[7] = -1; Batch b(q); expect_refusal(h, call(b), "target index of pair 3", 1); }
    EXPECT(std::string(teaser_hip_fgr_last_error(h)) == "corr: target index of pair 3 is outside the cloud (problem 1)");
    {
      Batch b(ps);
      expect_refusal(h, teaser_hip_fgr_correspondence_batch(h, B, b.src.data(), nullptr, b.dst.data(), b.nt.data(), b.corr.data(),
                                                            b.nc.data(), b.prm.data(), out.data()), "n_src", -1);
      expect_refusal(h, teaser_hip_fgr_correspondence_batch(h, B, b.src.data(), b.ns.data(), b.dst.data(), b.nt.data(),
                                                            b.corr.data(), b.nc.data(), nullptr, out.data()), "params", -1);
      expect_refusal(h, teaser_hip_fgr_correspondence_batch(h, B, b.src.data(), b.ns.data(), b.dst.data(), b.nt.data(),
                                                            b.corr.data(), b.nc.data(), b.prm.data(), nullptr), "out", -1);
      expect_refusal(h, teaser_hip_fgr_correspondence_batch(h, -1, b.src.data(), b.ns.data(), b.dst.data(), b.nt.data(),
                                                            b.corr.data(), b.nc.data(), b.prm.data(), out.data()), "batch", -1);
      EXPECT(teaser_hip_fgr_correspondence_batch(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                 nullptr) == TEASER_HIP_OK);
    }
    // the batch limit of the grids' y extent: 65 536 problems are refused by name before anything is read, allocated or
    // launched, by the full call and by the stage call
    {
      const int32_t big = 65536;
      const double pt[3] = {0.25, -1.0, 2.0};
      std::vector<const double*> one((size_t)big, pt);
      std::vector<const int32_t*> nc((size_t)big, nullptr);
      std::vector<int32_t> n1((size_t)big, 1), zero((size_t)big, 0);
      std::vector<teaser_fgr_params_c> prm((size_t)big, ps[0].prm);
      std::vector<teaser_fgr_result_c> wide((size_t)big);
      memset(wide.data(), 0x5a, sizeof(teaser_fgr_result_c) * wide.size());
      const std::vector<teaser_fgr_result_c> before = wide;
      const char* limit = "a batch holds at most 65535 problems; split larger batches across calls";
      EXPECT(teaser_hip_fgr_correspondence_batch(h, big, one.data(), n1.data(), one.data(), n1.data(), nc.data(), zero.data(),
                                                 prm.data(), wide.data()) == TEASER_HIP_ERR_UNSUPPORTED);
      EXPECT(std::string(teaser_hip_fgr_last_error(h)) == limit);
      EXPECT(memcmp(wide.data(), before.data(), sizeof(teaser_fgr_result_c) * wide.size()) == 0);
      EXPECT(teaser_hip_fgr_iterations_batch(h, big, one.data(), n1.data(), one.data(), n1.data(), nc.data(), zero.data(),
                                             prm.data(), 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                             nullptr, nullptr) == TEASER_HIP_ERR_UNSUPPORTED);
      EXPECT(std::string(teaser_hip_fgr_last_error(h)) == limit);
      // the stage call's n < 0 is refused before the batch is looked at: above the limit, empty or negative
      for (int32_t batch : {big, (int32_t)0, (int32_t)-1}) {
        EXPECT(teaser_hip_fgr_iterations_batch(h, batch, one.data(), n1.data(), one.data(), n1.data(), nc.data(), zero.data(),
                                               prm.data(), -1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG);
        EXPECT(std::string(teaser_hip_fgr_last_error(h)) == "n must be in 0 .. iteration_number");
      }
      EXPECT(teaser_hip_fgr_iterations_batch(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                                             nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_OK);
      EXPECT(std::string(teaser_hip_fgr_last_error(h)).empty());
    }
    EXPECT(g_normalise == norm0);  // nothing was launched by a refused call
    // ... and 65 535 one-point problems without correspondences pass it: every one comes back not optimised; the handle
    // is usable after the refusals
    {
      const int32_t most = 65535;
      const double pt[3] = {0.25, -1.0, 2.0};
      std::vector<const double*> one((size_t)most, pt);
      std::vector<const int32_t*> nc((size_t)most, nullptr);
      std::vector<int32_t> n1((size_t)most, 1), zero((size_t)most, 0);
      std::vector<teaser_fgr_params_c> prm((size_t)most, ps[0].prm);
      std::vector<teaser_fgr_result_c> wide((size_t)most);
      EXPECT(teaser_hip_fgr_correspondence_batch(h, most, one.data(), n1.data(), one.data(), n1.data(), nc.data(), zero.data(),
                                                 prm.data(), wide.data()) == TEASER_HIP_OK);
      EXPECT(std::string(teaser_hip_fgr_last_error(h)).empty());
      EXPECT(same(wide[0], wide[(size_t)most - 1]) && wide[0].iterations == 0 && wide[0].n_corr == 0);
    }
    const int norm1 = g_normalise;
    expect_refusal(h, teaser_hip_fgr_set_option(h, "resident_max_corr", 3073), "resident_max_corr must be in 0 .. 3072", -1);
    expect_refusal(h, teaser_hip_fgr_set_option(h, "resident_max_corr", -1), "resident_max_corr must be in 0 .. 3072", -1);
    expect_refusal(h, teaser_hip_fgr_set_option(h, "chunk_trials", 64), "unknown option chunk_trials", -1);
    auto said = [&](const char* text) { return std::string(teaser_hip_fgr_last_error(h)) == text; };
    EXPECT(teaser_hip_fgr_set_option(h, "resident_max_corr", 3073) == TEASER_HIP_ERR_BAD_ARG);
    EXPECT(said("resident_max_corr must be in 0 .. 3072"));
    EXPECT(teaser_hip_fgr_set_option(h, "no_such", 64) == TEASER_HIP_ERR_BAD_ARG && said("unknown option no_such"));
    EXPECT(teaser_hip_fgr_set_option(h, nullptr, 64) == TEASER_HIP_ERR_BAD_ARG && said("unknown option (NULL)"));
    EXPECT(teaser_hip_fgr_set_option(nullptr, "resident_max_corr", 64) == TEASER_HIP_ERR_BAD_ARG);
    // a failing get_option answers BAD_ARG, writes no value and leaves the handle's message as it was
    v = -5;
    EXPECT(teaser_hip_fgr_get_option(h, "nothing", &v) == TEASER_HIP_ERR_BAD_ARG && v == -5);
    EXPECT(teaser_hip_fgr_get_option(h, nullptr, &v) == TEASER_HIP_ERR_BAD_ARG && v == -5);
    EXPECT(teaser_hip_fgr_get_option(h, "resident_max_corr", nullptr) == TEASER_HIP_ERR_BAD_ARG);
    EXPECT(teaser_hip_fgr_get_option(nullptr, "resident_max_corr", &v) == TEASER_HIP_ERR_BAD_ARG && v == -5);
    EXPECT(said("unknown option (NULL)"));
    EXPECT(teaser_hip_fgr_get_option(h, "resident_max_corr", &v) == TEASER_HIP_OK && v == 3072);
    EXPECT(teaser_hip_fgr_params_default(nullptr) == TEASER_HIP_ERR_BAD_ARG);
    EXPECT(g_normalise == norm1);  // nothing was launched by a refused call
    EXPECT(std::string(teaser_hip_fgr_last_error(nullptr)).empty());
  }
  EXPECT(teaser_hip_fgr_destroy(h) == TEASER_HIP_OK);
  printf("normalise %d resident %d streamed steps %d moves %d finishes %d\nmismatches %d\n", g_normalise, g_resident,
         g_steps, g_moves, g_finishes, g_bad);
  return g_bad == 0 ? 0 : 1;
}
