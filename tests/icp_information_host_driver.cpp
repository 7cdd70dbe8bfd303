// Host-only check of csrc/icp_information.hip (tests/test_information_host.py): compiled by g++ against the HIP
// stand-in header (tests/hip_stub) with -fsanitize=address,undefined as a stand-alone program.  The launchers of the
// correspondence pass and of the reduction are stand-ins that walk the block map as the kernels do and read and write
// every row the kernels would: a buffer that is sized, packed or unpacked at a wrong offset is an AddressSanitizer
// report or a wrong value here.  Then the entry checks: every refusal names its argument and leaves the outputs alone.
//   icp_information_host_driver    exit code 0: every expectation met
// TEST INFRASTRUCTURE ONLY.
#define ICP_HOST_PRELUDE_OWN_ICP_LAUNCHERS
#include "icp_host_prelude.h"
#include "../teaser-plusplus_amd/csrc/icp.hip"
#include "../teaser-plusplus_amd/csrc/icp_information.hip"

#include <limits>

// coordinate c of point i of cloud p: small integers, so that every sum below is exact in any order
static double coord(int p, int i, int c) { return (double)((7 * p + 3 * i + 5 * c) % 23 - 11); }

static struct {
  int calls, n_blk, batch, mode, bad, info_calls;
} g_it;

// the 21 upper-triangle terms of G^T G at q, by rows
static void terms(const double* q, double* v) {
  const double G[3][6] = {{0, q[2], -q[1], 1, 0, 0}, {-q[2], 0, q[0], 0, 1, 0}, {q[1], -q[0], 0, 0, 0, 1}};
  int k = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c, ++k) v[k] = G[0][r] * G[0][c] + G[1][r] * G[1][c] + G[2][r] * G[2][c];
}

// source point i of a problem with n_t targets is matched with target (5 i) mod n_t, every third point with none
static int32_t match_of(int64_t i, int32_t n_t) { return n_t > 0 && i % 3 != 1 ? (int32_t)((5 * i) % n_t) : -1; }

namespace thip {

void launch_icp_covariances(hipStream_t, const IcpDesc*, const IcpCovDesc*, const int32_t*, int, int, const double*,
                            const double*, const int32_t*, const int32_t*, double*) {}

// One correspondence pass of the point-to-point instantiation: every source point looks at its own uploaded
// coordinates moved by U, at the index of its problem, writes its match; every block writes kIcpSums partials; the
// problem's state becomes what the finalize kernel leaves after a pass with max_iteration = 0.
void launch_icp_iteration(hipStream_t, const IcpDesc* desc, IcpState* state, const int32_t* blk_prob, int n_blk,
                          int batch, double* x, const double* qs, const int32_t* qj, const int32_t* bstart,
                          const double* normals, const double* cov_s, const double* cov_t, int mode, int32_t* match,
                          double* partials) {
  ++g_it.calls;
  g_it.n_blk = n_blk, g_it.batch = batch, g_it.mode = mode;
  g_it.bad += normals != nullptr || cov_s != nullptr || cov_t != nullptr;
  for (int blk = 0; blk < n_blk; ++blk) {
    const int p = blk_prob[blk];
    const IcpDesc& d = desc[p];
    g_it.bad += d.max_iteration != 0 || d.method != kIcpMethodPoint || state[p].done != 0 || state[p].phase != 0;
    for (int k = 0; k < kIcpSums; ++k) partials[(int64_t)kIcpSums * blk + k] = -1.0;
    for (int lane = 0; lane < kIcpBlock; ++lane) {
      const int64_t i = (int64_t)(blk - d.blk_off) * kIcpBlock + lane;
      if (i >= d.n_s) continue;
      g_it.bad += x[3 * (d.s_off + i) + 2] != coord(p, (int)i, 2);
      g_it.bad += state[p].U[3] != 100.0 + p || state[p].T[3] != 100.0 + p;
      if (d.n_t > 0) {
        const int64_t last = d.t_off + d.n_t - 1;
        g_it.bad += qj[last] < 0 || qj[last] >= d.n_t || !std::isfinite(qs[3 * last + 2]);
        g_it.bad += bstart[d.b_off + d.tb_mask + 1] != (int32_t)(d.t_off + d.n_t);
      }
      match[d.s_off + i] = match_of(i, d.n_t);
    }
  }
  for (int p = 0; p < batch; ++p) {
    int32_t cnt = 0;
    for (int64_t i = 0; i < desc[p].n_s; ++i) cnt += match_of(i, desc[p].n_t) >= 0;
    state[p].count = cnt;
    state[p].fitness = 0.5 + p;
    state[p].rmse = 0.25 + p;
    state[p].done = 1;
  }
}

// The reduction: per block the 21 sums over its matched points from the targets as given, per problem the sum of its
// blocks' partials.
void launch_icp_information(hipStream_t, const IcpDesc* desc, const int32_t* blk_prob, int n_blk, int batch,
                            const double* q, const int32_t* match, double* partials, double* info) {
  ++g_it.info_calls;
  g_it.bad += n_blk != g_it.n_blk || batch != g_it.batch;
  for (int blk = 0; blk < n_blk; ++blk) {
    const int p = blk_prob[blk];
    const IcpDesc& d = desc[p];
    double* pb = partials + (int64_t)kIcpInfoSums * blk;
    for (int k = 0; k < kIcpInfoSums; ++k) pb[k] = 0.0;
    for (int lane = 0; lane < kIcpBlock; ++lane) {
      const int64_t i = (int64_t)(blk - d.blk_off) * kIcpBlock + lane;
      if (i >= d.n_s || match[d.s_off + i] < 0) continue;
      double v[kIcpInfoSums];
      terms(q + 3 * (d.t_off + match[d.s_off + i]), v);
      for (int k = 0; k < kIcpInfoSums; ++k) pb[k] += v[k];
    }
  }
  for (int p = 0; p < batch; ++p) {
    const IcpDesc& d = desc[p];
    double tot[kIcpInfoSums] = {};
    for (int b = 0; b < d.nblk; ++b)
      for (int k = 0; k < kIcpInfoSums; ++k) tot[k] += partials[(int64_t)kIcpInfoSums * (d.blk_off + b) + k];
    int k = 0;
    for (int r = 0; r < 6; ++r)
      for (int c = r; c < 6; ++c, ++k) info[36 * p + 6 * r + c] = info[36 * p + 6 * c + r] = tot[k];
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

  // ---- sizing, packing and unpacking at the block edges of kIcpBlock = 256, with empty problems in the batch ----
  {
    constexpr int B = 6;
    const int32_t n_src[B] = {0, 1, 255, 256, 257, 700}, n_dst[B] = {5, 0, 1, 65, 257, 64};
    std::vector<std::vector<double>> src, dst;
    for (int b = 0; b < B; ++b) src.push_back(cloud(b, n_src[b])), dst.push_back(cloud(b + B, n_dst[b]));
    const double* ps[B];
    const double* pd[B];
    for (int b = 0; b < B; ++b) ps[b] = n_src[b] ? src[(size_t)b].data() : nullptr, pd[b] = n_dst[b] ? dst[(size_t)b].data() : nullptr;
    double T[16 * B], r[B];
    for (int b = 0; b < B; ++b) {
      const double eye[16] = {1, 0, 0, 100.0 + b, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
      memcpy(T + 16 * b, eye, sizeof(eye));
      r[b] = 0.5 + b;
    }
    int want_blk = 0;
    for (int b = 0; b < B; ++b) want_blk += (n_src[b] + kIcpBlock - 1) / kIcpBlock;
    for (int round = 0; round < 3; ++round) {  // without out / corr, with out, with out and corr (on grown buffers)
      std::vector<double> info(36 * B, -3.0);
      teaser_icp_result_c out[B];
      memset(out, 0xff, sizeof(out));
      std::vector<std::vector<int32_t>> corr;
      for (int b = 0; b < B; ++b) corr.emplace_back(2 * (size_t)std::max(n_src[b], 1), -7);
      int32_t* pc[B];
      for (int b = 0; b < B; ++b) pc[b] = b == 2 ? nullptr : corr[(size_t)b].data();  // a problem may decline
      g_it = {};
      expect(teaser_hip_icp_information_batch(h, B, ps, n_src, pd, n_dst, T, r, info.data(), round >= 1 ? out : nullptr,
                                              round >= 2 ? pc : nullptr) == TEASER_HIP_OK,
             teaser_hip_icp_last_error(h), round);
      expect(g_it.calls == 1 && g_it.info_calls == 1, "one correspondence pass, one reduction", round);
      expect(g_it.n_blk == want_blk && g_it.batch == B && g_it.mode == 0, "the point-to-point launch over every block",
             round);
      expect(g_it.bad == 0, "a launch saw a row or a record that is not its own", round);
      for (int b = 0; b < B; ++b) {
        double tot[kIcpInfoSums] = {};
        int32_t cnt = 0;
        for (int i = 0; i < n_src[b]; ++i) {
          const int32_t j = match_of(i, n_dst[b]);
          if (j < 0) continue;
          double v[kIcpInfoSums];
          terms(&dst[(size_t)b][3 * (size_t)j], v);
          for (int k = 0; k < kIcpInfoSums; ++k) tot[k] += v[k];
          if (round >= 2 && pc[b])
            expect(corr[(size_t)b][2 * (size_t)cnt] == i && corr[(size_t)b][2 * (size_t)cnt + 1] == j,
                   "a correspondence of another point", b);
          ++cnt;
        }
        int k = 0;
        for (int rr = 0; rr < 6; ++rr)
          for (int c = rr; c < 6; ++c, ++k)
            expect(info[36 * (size_t)b + 6 * rr + c] == tot[k] && info[36 * (size_t)b + 6 * c + rr] == tot[k],
                   "information: an entry of another problem", b);
        expect(info[36 * (size_t)b + 35] == cnt, "information(5,5) is the number of correspondences", b);
        if (round >= 1) {
          expect(out[b].n_correspondences == cnt && out[b].iterations == 0 && out[b].fitness == 0.5 + b &&
                     out[b].inlier_rmse == 0.25 + b,
                 "out: the record of another problem", b);
          expect(memcmp(out[b].transformation, T + 16 * b, 128) == 0, "out: the transformation is echoed", b);
        }
        if (round >= 2 && pc[b] && (size_t)(2 * cnt) < corr[(size_t)b].size())
          expect(corr[(size_t)b][2 * (size_t)cnt] == -7, "corr: written past the last pair", b);
      }
    }
    // one problem through the single form gives the row of the batch
    std::vector<double> one(36, -3.0), all(36 * B, -3.0);
    expect(teaser_hip_icp_information_batch(h, B, ps, n_src, pd, n_dst, T, r, all.data(), nullptr, nullptr) == TEASER_HIP_OK,
           teaser_hip_icp_last_error(h), 10);
    expect(teaser_hip_icp_information(h, ps[4], n_src[4], pd[4], n_dst[4], T + 64, r[4], one.data(), nullptr, nullptr) ==
               TEASER_HIP_OK,
           teaser_hip_icp_last_error(h), 10);
    for (int k = 0; k < 36; ++k) expect(one[(size_t)k] == all[36 * 4 + (size_t)k], "the one-problem form", 10);
  }

  // ---- entry checks: BAD_ARG, the argument named, the outputs untouched, the handle usable afterwards ----
  {
    const std::vector<double> p = cloud(1, 4), q = cloud(2, 3);
    const double* ps[1] = {p.data()};
    const double* pd[1] = {q.data()};
    const int32_t ns[1] = {4}, nd[1] = {3};
    const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const double r[1] = {1.0};
    double info[36];
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    auto refused = [&](int32_t rc, const char* word, int c) {
      expect(rc == TEASER_HIP_ERR_BAD_ARG, "a bad argument is refused", c);
      expect(strstr(teaser_hip_icp_last_error(h), word) != nullptr, "the refusal names its argument", c);
      expect(info[0] == -3.0 && info[35] == -3.0, "a refusal leaves information alone", c);
    };
    for (double& v : info) v = -3.0;
    expect(teaser_hip_icp_information_batch(nullptr, 1, ps, ns, pd, nd, eye, r, info, nullptr, nullptr) ==
               TEASER_HIP_ERR_BAD_ARG, "a NULL handle", 20);
    refused(teaser_hip_icp_information_batch(h, -1, ps, ns, pd, nd, eye, r, info, nullptr, nullptr), "batch", 21);
    refused(teaser_hip_icp_information_batch(h, 1, ps, nullptr, pd, nd, eye, r, info, nullptr, nullptr), "n_src", 22);
    refused(teaser_hip_icp_information_batch(h, 1, ps, ns, pd, nullptr, eye, r, info, nullptr, nullptr), "n_dst", 23);
    refused(teaser_hip_icp_information_batch(h, 1, ps, ns, pd, nd, nullptr, r, info, nullptr, nullptr), "transformation", 24);
    refused(teaser_hip_icp_information_batch(h, 1, ps, ns, pd, nd, eye, nullptr, info, nullptr, nullptr),
            "max_correspondence_distance", 25);
    expect(teaser_hip_icp_information_batch(h, 1, ps, ns, pd, nd, eye, r, nullptr, nullptr, nullptr) ==
               TEASER_HIP_ERR_BAD_ARG && strstr(teaser_hip_icp_last_error(h), "information"), "a NULL information", 26);
    refused(teaser_hip_icp_information_batch(h, 1, nullptr, ns, pd, nd, eye, r, info, nullptr, nullptr), "src", 27);
    const double* none[1] = {nullptr};
    refused(teaser_hip_icp_information_batch(h, 1, ps, ns, none, nd, eye, r, info, nullptr, nullptr), "dst", 28);
    const int32_t neg[1] = {-1};
    refused(teaser_hip_icp_information_batch(h, 1, ps, neg, pd, nd, eye, r, info, nullptr, nullptr), "n_src", 29);
    for (double bad_r : {0.0, -1.0, nan, inf, 1e200, 1e-200}) {
      const double rr[1] = {bad_r};
      refused(teaser_hip_icp_information_batch(h, 1, ps, ns, pd, nd, eye, rr, info, nullptr, nullptr),
              "max_correspondence_distance", 30);
    }
    for (int k = 0; k < 16; ++k) {
      double T[16];
      memcpy(T, eye, sizeof(T));
      T[k] = k % 2 ? nan : inf;
      refused(teaser_hip_icp_information_batch(h, 1, ps, ns, pd, nd, T, r, info, nullptr, nullptr), "transformation", 31);
    }
    for (int k = 12; k < 16; ++k) {
      double T[16];
      memcpy(T, eye, sizeof(T));
      T[k] = 0.5;
      refused(teaser_hip_icp_information_batch(h, 1, ps, ns, pd, nd, T, r, info, nullptr, nullptr), "last row", 32);
    }
    std::vector<double> pbad = p, qbad = q;
    pbad[5] = nan, qbad[2] = inf;
    const double* pb[1] = {pbad.data()};
    const double* qb[1] = {qbad.data()};
    refused(teaser_hip_icp_information_batch(h, 1, pb, ns, pd, nd, eye, r, info, nullptr, nullptr), "src", 33);
    refused(teaser_hip_icp_information_batch(h, 1, ps, ns, qb, nd, eye, r, info, nullptr, nullptr), "dst", 34);
    // the second problem of a batch is named as problem 1
    const double* ps2[2] = {p.data(), p.data()};
    const double* pd2[2] = {q.data(), q.data()};
    const int32_t ns2[2] = {4, 4}, nd2[2] = {3, 3};
    double T2[32], r2[2] = {1.0, 1.0};
    memcpy(T2, eye, sizeof(eye)), memcpy(T2 + 16, eye, sizeof(eye));
    T2[16 + 15] = 2.0;
    double info2[72];
    expect(teaser_hip_icp_information_batch(h, 2, ps2, ns2, pd2, nd2, T2, r2, info2, nullptr, nullptr) ==
               TEASER_HIP_ERR_BAD_ARG && strstr(teaser_hip_icp_last_error(h), "problem 1"), "the problem is named", 35);
    // valid: batch 0 touches nothing; n = 0 with NULL clouds is the zero matrix; the handle still serves
    expect(teaser_hip_icp_information_batch(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                            nullptr) == TEASER_HIP_OK, "batch 0", 36);
    const int32_t zero[1] = {0};
    teaser_icp_result_c out;
    expect(teaser_hip_icp_information_batch(h, 1, nullptr, zero, nullptr, zero, eye, r, info, &out, nullptr) ==
               TEASER_HIP_OK, teaser_hip_icp_last_error(h), 37);
    for (double v : info) expect(v == 0.0, "n = 0 gives the zero matrix", 37);
    expect(out.n_correspondences == 0 && out.iterations == 0, "n = 0: no correspondences", 37);
    expect(teaser_hip_icp_last_error(h)[0] == 0, "a successful call clears the message", 37);
  }
  teaser_hip_icp_destroy(h);
  std::printf("mismatches %d\n", g_bad);
  return g_bad ? 1 : 0;
}
