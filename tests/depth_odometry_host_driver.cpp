// Host-only check of depth odometry (tests/test_depth_odometry_host.py): csrc/icp_depth_odometry.hip compiled by g++
// against the HIP stand-in header (tests/hip_stub), built with -ffp-contract=off -fsanitize=address,undefined as a
// stand-alone program.  The launchers are serial loops over the functions of csrc/icp_depth_odometry_device.h -- the text
// the kernels compile -- walking the block map, the blocks' pixels and the summation tree exactly as the kernels do.
// "Device" buffers are host allocations of the size the host code asked for and every image of a case is an allocation
// that ends with its last row's last sample, so a record, an offset, a row stride or an output layout that is sized or
// addressed wrongly is an AddressSanitizer report.  Pyramids, traces, transformations, information matrices, measures and
// counts are compared for equality with those of tests/depth_odometry_reference.py, read from a text file (hexadecimal
// floats).
//   depth_odometry_host_driver CASES.txt      exit code 0: every case equal and every refusal refused
// TEST INFRASTRUCTURE ONLY.
#include <functional>

#include "icp_host_prelude.h"
#include "../teaser-plusplus_amd/csrc/icp.hip"
#include "../teaser-plusplus_amd/csrc/icp_depth_odometry.hip"

static int g_launches = 0;
static void expects(bool ok, const std::string& what, int c) { expect(ok, what.c_str(), c); }

namespace thip {

// fn(pair, pixel) for every thread of the launch over level l that is inside its pair's level, in block order
static void for_each_pixel(const DodoArgs& a, int l, const std::function<void(int, int32_t)>& fn) {
  for (int blk = 0; blk < a.level_nblk[l]; ++blk) {
    const int p = a.blk_pair[a.level_blk0[l] + blk];
    if (p < 0 || p >= a.batch || blk < a.desc[p].blk_off[l]) std::abort();
    for (int t = 0; t < kOdoBlock; ++t) {
      const int32_t px = (blk - a.desc[p].blk_off[l]) * kOdoBlock + t;
      if (px < dodo_n(a.desc[p], l)) fn(p, px);
    }
  }
}

static void host_sums_and_finish(const DodoArgs& a, int mode, int l, int iter, int first, int last) {
  ++g_launches;
  for (int blk = 0; blk < a.level_nblk[l]; ++blk) {
    const int p = a.blk_pair[a.level_blk0[l] + blk];
    const DodoDesc& d = a.desc[p];
    if (a.state[p].failed || (mode == kDodoSumIter && a.state[p].converged)) continue;
    static double v[kOdoBlock][kOdoSums];
    for (int t = 0; t < kOdoBlock; ++t) {
      const int64_t s = (int64_t)(blk - d.blk_off[l]) * kOdoBlock + t;
      dodo_px_values(mode, d, a.state[p], a.img, l, s, s < dodo_n(d, l), v[t]);
    }
    for (int k = 0; k < kOdoSums; ++k) {
      double run[4];
      for (int w = 0; w < 4; ++w) {
        double s[64];
        for (int i = 0; i < 64; ++i) s[i] = v[64 * w + i][k];
        for (int o = 32; o > 0; o >>= 1)
          for (int i = 0; i < o; ++i) s[i] = s[i] + s[i + o];
        run[w] = s[0];
      }
      a.part[(d.part_off + (blk - d.blk_off[l])) * kOdoSums + k] = (run[0] + run[1]) + (run[2] + run[3]);
    }
  }
  ++g_launches;
  for (int p = 0; p < a.batch; ++p) {
    const DodoDesc& d = a.desc[p];
    DodoState& st = a.state[p];
    const bool failed = st.failed != 0;
    if (mode == kDodoSumIter) {
      if (failed) continue;
      if (st.converged) {
        if (last) st.converged = 0;
        continue;
      }
    }
    double tot[kOdoSums];
    for (int k = 0; k < kOdoSums; ++k) tot[k] = failed ? 0.0 : odo_sum_blocks(a.part + d.part_off * kOdoSums, dodo_blocks(d, l), k);
    teaser_icp_depth_odometry_trace_c* rec = (mode == kDodoSumIter && d.trace_off >= 0) ? a.trace + d.trace_off + iter : nullptr;
    dodo_finish(mode, d, st, tot, l, first, a.results + p, rec);
    if (mode == kDodoSumIter && last) st.converged = 0;
  }
}

void launch_dodo_preprocess(hipStream_t, const DodoArgs& a) {
  ++g_launches;
  for_each_pixel(a, 0, [&](int p, int32_t px) {
    const DodoDesc& d = a.desc[p];
    dodo_px_convert(d, a.in, a.img, 0, px / d.width, px % d.width);
    dodo_px_convert(d, a.in, a.img, 1, px / d.width, px % d.width);
  });
  for (int l = 0; l + 1 < a.levels; ++l) {
    ++g_launches;
    for_each_pixel(a, l + 1, [&](int p, int32_t px) {
      const int w = dodo_w(a.desc[p], l + 1);
      dodo_px_down(a.desc[p], a.img, l, 0, px / w, px % w);
      dodo_px_down(a.desc[p], a.img, l, 1, px / w, px % w);
    });
  }
  ++g_launches;
  for (int l = 0; l < a.levels; ++l)
    for_each_pixel(a, l, [&](int p, int32_t px) {
      const int w = dodo_w(a.desc[p], l);
      dodo_px_vertex(a.desc[p], a.img, l, 0, px / w, px % w);
      dodo_px_vertex(a.desc[p], a.img, l, 1, px / w, px % w);
    });
  ++g_launches;
  for (int l = 0; l < a.levels; ++l)
    for_each_pixel(a, l, [&](int p, int32_t px) {
      const int w = dodo_w(a.desc[p], l);
      dodo_px_normal(a.desc[p], a.img, l, px / w, px % w);
    });
}

void launch_dodo_iteration(hipStream_t, const DodoArgs& a, int level, int iter, int first, int last) {
  host_sums_and_finish(a, kDodoSumIter, level, iter, first, last);
}

void launch_dodo_information(hipStream_t, const DodoArgs& a) { host_sums_and_finish(a, kDodoSumInfo, 0, 0, 0, 0); }

}  // namespace thip

// rows of `row` bytes, `pad` bytes of 0xAB between them, `comp` bytes per number: 2 uint16, 4 float32
static void read_image(FILE* f, std::vector<unsigned char>& img, int64_t h, int64_t row, int64_t pad, int comp) {
  img.assign((size_t)((h - 1) * (row + pad) + row), 0xAB);
  for (int64_t i = 0; i < h; ++i)
    for (int64_t k = 0; k < row / comp; ++k) {
      const double v = read_number(f);
      unsigned char* at = img.data() + i * (row + pad) + k * comp;
      if (comp == 2) {
        const uint16_t s = (uint16_t)v;
        memcpy(at, &s, 2);
      } else {
        const float s = (float)v;
        memcpy(at, &s, 4);
      }
    }
}

struct Case {
  teaser_icp_depth_odometry_pair_c pair;
  teaser_icp_depth_odometry_option_c opt;
  std::vector<unsigned char> img[2];
  std::vector<float> pyramid;
  teaser_icp_depth_odometry_result_c res;
  std::vector<teaser_icp_depth_odometry_trace_c> trace;
  int n_iter = 0;
};

static uint32_t bits32(float x) {
  uint32_t b;
  memcpy(&b, &x, 4);
  return b;
}
static bool same_doubles(const double* a, const double* b, size_t n) { return memcmp(a, b, 8 * n) == 0; }

static bool same_result(const teaser_icp_depth_odometry_result_c& a, const teaser_icp_depth_odometry_result_c& b) {
  return a.success == b.success && a.count == b.count && a.iterations == b.iterations && a.converged_levels == b.converged_levels &&
         same_doubles(&a.fitness, &b.fitness, 1) && same_doubles(&a.inlier_rmse, &b.inlier_rmse, 1) &&
         same_doubles(a.transformation, b.transformation, 16) && same_doubles(a.information, b.information, 36);
}
static bool same_trace(const teaser_icp_depth_odometry_trace_c& a, const teaser_icp_depth_odometry_trace_c& b) {
  return a.level == b.level && a.executed == b.executed && a.count == b.count && a.failed == b.failed && a.converged == b.converged &&
         a.reserved == 0 && same_doubles(&a.e, &b.e, 1) && same_doubles(a.A, b.A, 21) && same_doubles(a.g, b.g, 6) &&
         same_doubles(a.pose, b.pose, 16) && a.reserved2 == 0.0;
}

struct Batch {
  std::vector<teaser_icp_depth_odometry_pair_c> pairs;
  std::vector<const void*> p[2];
  void add(const Case& cs) {
    pairs.push_back(cs.pair);
    for (int k = 0; k < 2; ++k) p[k].push_back(cs.img[k].data());
  }
};

static void refused(teaser_hip_icp* h, int32_t rc, const char* w1, const char* w2) {
  const std::string msg = h->err;
  expects(rc == TEASER_HIP_ERR_BAD_ARG && msg.find(w1) != std::string::npos && msg.find(w2) != std::string::npos,
          std::string("refusal: ") + w1 + " / " + msg, -1);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const int nc = (int)read_number(f);
  std::vector<Case> cases((size_t)nc);
  for (Case& cs : cases) {
    memset(&cs.pair, 0, sizeof(cs.pair));
    if (teaser_hip_icp_depth_odometry_option_default(&cs.opt) != TEASER_HIP_OK) return 2;
    teaser_icp_depth_odometry_pair_c& p = cs.pair;
    p.width = (int)read_number(f), p.height = (int)read_number(f), p.depth_format = (int)read_number(f);
    const int64_t pad = (int64_t)read_number(f);
    cs.opt.n_levels = (int)read_number(f);
    memset(cs.opt.iterations, 0, sizeof(cs.opt.iterations));
    for (int k = 0; k < cs.opt.n_levels; ++k) cs.n_iter += (cs.opt.iterations[k] = (int)read_number(f));
    p.fx = read_number(f), p.fy = read_number(f), p.cx = read_number(f), p.cy = read_number(f);
    for (double& m : p.init) m = read_number(f);
    p.depth_scale = read_number(f);
    cs.opt.depth_outlier_trunc = read_number(f), cs.opt.depth_huber_delta = read_number(f);
    cs.opt.depth_min = read_number(f), cs.opt.depth_max = read_number(f);
    cs.opt.relative_rmse = read_number(f), cs.opt.relative_fitness = read_number(f);
    const int comp = p.depth_format == 0 ? 2 : 4;
    const int64_t row = (int64_t)p.width * comp;
    p.source_depth_row_bytes = p.target_depth_row_bytes = row + pad;
    for (int k = 0; k < 2; ++k) read_image(f, cs.img[k], p.height, row, pad, comp);
    cs.pyramid.resize((size_t)(thip::kDodoPlanes * thip::odo_pyramid_pixels(p.width, p.height, cs.opt.n_levels)));
    for (float& x : cs.pyramid) x = (float)read_number(f);
    memset(&cs.res, 0, sizeof(cs.res));
    cs.res.success = (int)read_number(f), cs.res.count = (int)read_number(f), cs.res.iterations = (int)read_number(f);
    cs.res.converged_levels = (int)read_number(f);
    cs.res.fitness = read_number(f), cs.res.inlier_rmse = read_number(f);
    for (double& m : cs.res.transformation) m = read_number(f);
    for (double& m : cs.res.information) m = read_number(f);
    cs.trace.resize((size_t)cs.n_iter);
    for (teaser_icp_depth_odometry_trace_c& t : cs.trace) {
      memset(&t, 0, sizeof(t));
      t.level = (int)read_number(f), t.executed = (int)read_number(f), t.count = (int)read_number(f), t.failed = (int)read_number(f);
      t.converged = (int)read_number(f);
      t.e = read_number(f);
      for (double& m : t.A) m = read_number(f);
      for (double& m : t.g) m = read_number(f);
      for (double& m : t.pose) m = read_number(f);
    }
  }
  std::fclose(f);

  teaser_hip_icp* h = nullptr;
  if (teaser_hip_icp_create(0, &h) != TEASER_HIP_OK) return 2;
  // every case alone: the pyramid stage, then the odometry with its trace
  for (int c = 0; c < nc; ++c) {
    const Case& cs = cases[(size_t)c];
    Batch one;
    one.add(cs);
    std::vector<float> pyr(cs.pyramid.size() + 1, -7.5f);
    float* out = pyr.data();
    g_launches = 0;
    expects(teaser_hip_icp_depth_odometry_pyramid_pairs(h, 1, one.pairs.data(), &cs.opt, one.p[0].data(), one.p[1].data(), &out) ==
                TEASER_HIP_OK, "pyramid: " + h->err, c);
    expects(g_launches == cs.opt.n_levels + 2, "the pyramid stage is convert, L - 1 steps down, vertex, normal", c);
    size_t diff = 0, first = 0;
    for (size_t k = 0; k < cs.pyramid.size(); ++k)
      if (bits32(pyr[k]) != bits32(cs.pyramid[k]) && diff++ == 0) first = k;
    expects(diff == 0, "pyramid bits: " + std::to_string(diff) + " differ, the first at float " + std::to_string(first), c);
    expects(pyr.back() == -7.5f, "a float behind the pyramid is written", c);
    teaser_icp_depth_odometry_result_c res;
    memset(&res, 0xCD, sizeof(res));
    std::vector<teaser_icp_depth_odometry_trace_c> tr((size_t)cs.n_iter + 1);
    memset(tr.data(), 0xCD, sizeof(tr[0]) * tr.size());
    teaser_icp_depth_odometry_trace_c* trp = tr.data();
    g_launches = 0;
    expects(teaser_hip_icp_depth_odometry_pairs(h, 1, one.pairs.data(), &cs.opt, one.p[0].data(), one.p[1].data(), &res, &trp) ==
                TEASER_HIP_OK, "odometry: " + h->err, c);
    // preprocessing L + 2, two per iteration, two for the information matrix: whatever fails or converges
    expects(g_launches == cs.opt.n_levels + 2 + 2 * cs.n_iter + 2, "the launch count follows from the options alone", c);
    expects(same_result(res, cs.res), "result bits", c);
    for (int k = 0; k < cs.n_iter; ++k) expects(same_trace(tr[(size_t)k], cs.trace[(size_t)k]), "trace record " + std::to_string(k), c);
    expects(((unsigned char*)&tr[(size_t)cs.n_iter])[0] == 0xCD, "a record behind the trace is written", c);
  }
  // all cases with the same options in one call, in reverse order, without traces for every other pair: the same bits
  for (int c0 = 0; c0 < nc; ++c0) {
    std::vector<int> group;
    for (int c = nc - 1; c >= 0; --c)
      if (memcmp(&cases[(size_t)c].opt, &cases[(size_t)c0].opt, sizeof(cases[0].opt)) == 0) group.push_back(c);
    if (group.back() != c0 || group.size() < 2) continue;  // once per group
    Batch all;
    for (int c : group) all.add(cases[(size_t)c]);
    const int b = (int)group.size(), n_iter = cases[(size_t)c0].n_iter;
    std::vector<teaser_icp_depth_odometry_result_c> res((size_t)b);
    std::vector<std::vector<teaser_icp_depth_odometry_trace_c>> tr((size_t)b, std::vector<teaser_icp_depth_odometry_trace_c>((size_t)n_iter + 1));
    std::vector<teaser_icp_depth_odometry_trace_c*> trp;
    for (int k = 0; k < b; ++k) trp.push_back(k % 2 == 0 ? tr[(size_t)k].data() : nullptr);
    expects(teaser_hip_icp_depth_odometry_pairs(h, b, all.pairs.data(), &cases[(size_t)c0].opt, all.p[0].data(), all.p[1].data(), res.data(),
                                                trp.data()) == TEASER_HIP_OK, "batch: " + h->err, c0);
    std::vector<std::vector<float>> pyr;
    std::vector<float*> pp;
    for (int c : group) pyr.emplace_back(cases[(size_t)c].pyramid.size(), -7.5f);
    for (auto& v : pyr) pp.push_back(v.data());
    expects(teaser_hip_icp_depth_odometry_pyramid_pairs(h, b, all.pairs.data(), &cases[(size_t)c0].opt, all.p[0].data(), all.p[1].data(),
                                                        pp.data()) == TEASER_HIP_OK, "pyramid batch: " + h->err, c0);
    for (int k = 0; k < b; ++k) {
      const Case& cs = cases[(size_t)group[(size_t)k]];
      expects(same_result(res[(size_t)k], cs.res), "result bits in a batch", group[(size_t)k]);
      expects(memcmp(pyr[(size_t)k].data(), cs.pyramid.data(), 4 * cs.pyramid.size()) == 0, "pyramid bits in a batch", group[(size_t)k]);
      if (k % 2 == 0)
        for (int i = 0; i < n_iter; ++i) expects(same_trace(tr[(size_t)k][(size_t)i], cs.trace[(size_t)i]), "trace in a batch", group[(size_t)k]);
    }
  }

  // refusals: BAD_ARG with the argument (and the pair) named; the handle stays usable
  const Case& c0 = cases[0];
  Batch two;
  two.add(c0);
  two.add(c0);
  teaser_icp_depth_odometry_result_c res[2];
  typedef teaser_icp_depth_odometry_pair_c PR;
  typedef teaser_icp_depth_odometry_option_c OP;
  auto call = [&](int which, void (*change)(PR&), void (*change_opt)(OP&)) {
    std::vector<PR> pr = two.pairs;
    OP o = c0.opt;
    if (change) change(pr[(size_t)which]);
    if (change_opt) change_opt(o);
    return teaser_hip_icp_depth_odometry_pairs(h, 2, pr.data(), &o, two.p[0].data(), two.p[1].data(), res, nullptr);
  };
  refused(h, call(1, [](PR& x) { x.depth_format = 2; }, nullptr), "depth_format", "pair 1");
  refused(h, call(0, [](PR& x) { x.depth_format = -1; }, nullptr), "depth_format", "pair 0");
  refused(h, call(1, [](PR& x) { x.reserved = 1; }, nullptr), "reserved", "pair 1");
  refused(h, call(0, [](PR& x) { x.reserved2 = 1.0; }, nullptr), "reserved", "pair 0");
  refused(h, call(1, [](PR& x) { x.width = 0; }, nullptr), "every level needs a pixel", "pair 1");
  refused(h, call(0, [](PR& x) { x.height = 16385; }, nullptr), "width and height", "pair 0");
  refused(h, call(0, [](PR& x) { x.fx = 0.0; }, nullptr), "fx and fy", "pair 0");
  refused(h, call(1, [](PR& x) { x.fy = -1.0; }, nullptr), "fx and fy", "pair 1");
  refused(h, call(1, [](PR& x) { x.fx = NAN; }, nullptr), "fx and fy", "pair 1");
  refused(h, call(0, [](PR& x) { x.cy = INFINITY; }, nullptr), "cx and cy", "pair 0");
  refused(h, call(1, [](PR& x) { x.init[6] = NAN; }, nullptr), "init has a non-finite entry", "pair 1");
  refused(h, call(0, [](PR& x) { x.depth_scale = 0.0; }, nullptr), "depth_scale", "pair 0");
  refused(h, call(1, [](PR& x) { x.source_depth_row_bytes = 1; }, nullptr), "source_depth_row_bytes", "pair 1");
  refused(h, call(0, [](PR& x) { x.target_depth_row_bytes = 1; }, nullptr), "target_depth_row_bytes", "pair 0");
  refused(h, call(0, nullptr, [](OP& o) { o.n_levels = 0; }), "n_levels", "");
  refused(h, call(0, nullptr, [](OP& o) { o.n_levels = 9; }), "n_levels", "");
  refused(h, call(0, nullptr, [](OP& o) { o.iterations[0] = -1; }), "iterations", "entry 0");
  refused(h, call(0, nullptr, [](OP& o) { o.reserved[2] = 1; }), "reserved", "option");
  refused(h, call(0, nullptr, [](OP& o) { o.reserved2[1] = 1.0; }), "reserved", "option");
  refused(h, call(0, nullptr, [](OP& o) { o.depth_outlier_trunc = 0.0; }), "depth_outlier_trunc must be finite and > 0", "");
  refused(h, call(0, nullptr, [](OP& o) { o.depth_outlier_trunc = NAN; }), "depth_outlier_trunc must be finite and > 0", "");
  refused(h, call(0, nullptr, [](OP& o) { o.depth_huber_delta = -1.0; }), "depth_huber_delta must be finite and > 0", "");
  refused(h, call(0, nullptr, [](OP& o) { o.depth_huber_delta = INFINITY; }), "depth_huber_delta must be finite and > 0", "");
  refused(h, call(0, nullptr, [](OP& o) { o.depth_min = INFINITY; }), "depth_min", "");
  refused(h, call(0, nullptr, [](OP& o) { o.depth_min = -0.5; }), "depth_min", "");
  refused(h, call(0, nullptr, [](OP& o) { o.depth_max = NAN; }), "depth_max", "");
  refused(h, call(0, nullptr, [](OP& o) { o.relative_rmse = NAN; }), "relative_rmse must be finite", "");
  refused(h, call(0, nullptr, [](OP& o) { o.relative_fitness = INFINITY; }), "relative_fitness must be finite", "");
  const void* half[2] = {c0.img[1].data(), nullptr};
  refused(h, teaser_hip_icp_depth_odometry_pairs(h, 2, two.pairs.data(), &c0.opt, two.p[0].data(), half, res, nullptr), "target_depth is NULL", "pair 1");
  refused(h, teaser_hip_icp_depth_odometry_pairs(h, 2, two.pairs.data(), &c0.opt, nullptr, two.p[1].data(), res, nullptr),
          "source_depth must not be NULL", "");
  refused(h, teaser_hip_icp_depth_odometry_pairs(h, 2, nullptr, &c0.opt, two.p[0].data(), two.p[1].data(), res, nullptr), "pairs must not be NULL", "");
  refused(h, teaser_hip_icp_depth_odometry_pairs(h, 2, two.pairs.data(), nullptr, two.p[0].data(), two.p[1].data(), res, nullptr),
          "option must not be NULL", "");
  refused(h, teaser_hip_icp_depth_odometry_pairs(h, 2, two.pairs.data(), &c0.opt, two.p[0].data(), two.p[1].data(), nullptr, nullptr),
          "results must not be NULL", "");
  refused(h, teaser_hip_icp_depth_odometry_pairs(h, -1, two.pairs.data(), &c0.opt, two.p[0].data(), two.p[1].data(), res, nullptr), "batch", "");
  refused(h, teaser_hip_icp_depth_odometry_pyramid_pairs(h, 2, two.pairs.data(), &c0.opt, two.p[0].data(), two.p[1].data(), nullptr),
          "images_out must not be NULL", "");
  float* none[2] = {nullptr, nullptr};
  refused(h, teaser_hip_icp_depth_odometry_pyramid_pairs(h, 2, two.pairs.data(), &c0.opt, two.p[0].data(), two.p[1].data(), none),
          "images_out is NULL", "pair 0");
  expects(teaser_hip_icp_depth_odometry_pairs(nullptr, 2, two.pairs.data(), &c0.opt, two.p[0].data(), two.p[1].data(), res, nullptr) ==
                  TEASER_HIP_ERR_BAD_ARG && teaser_hip_icp_depth_odometry_option_default(nullptr) == TEASER_HIP_ERR_BAD_ARG, "refusal: NULL handle", -1);
  g_launches = 0;
  expects(teaser_hip_icp_depth_odometry_pairs(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_OK &&
              teaser_hip_icp_depth_odometry_pyramid_pairs(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_OK && g_launches == 0,
          "an empty batch does nothing", -1);
  teaser_icp_depth_odometry_option_c d;
  memset(&d, 0x5A, sizeof(d));
  expects(teaser_hip_icp_depth_odometry_option_default(&d) == TEASER_HIP_OK && d.n_levels == 3 && d.iterations[0] == 10 && d.iterations[1] == 5 &&
              d.iterations[2] == 3 && d.iterations[3] == 0 && d.depth_outlier_trunc == 0.07 && d.depth_huber_delta == 0.05 && d.depth_min == 0.0 &&
              d.depth_max == 3.0 && d.relative_rmse == 1e-6 && d.relative_fitness == 1e-6 && d.reserved2[0] == 0.0 && d.reserved2[1] == 0.0,
          "defaults", -1);
  // the handle works afterwards
  expects(teaser_hip_icp_depth_odometry_pairs(h, 2, two.pairs.data(), &c0.opt, two.p[0].data(), two.p[1].data(), res, nullptr) == TEASER_HIP_OK &&
              same_result(res[0], c0.res) && same_result(res[1], c0.res), "the handle works after the refusals", -1);
  teaser_hip_icp_destroy(h);
  std::printf("cases %d  mismatches %d\n", nc, g_bad);
  return g_bad ? 1 : 0;
}
