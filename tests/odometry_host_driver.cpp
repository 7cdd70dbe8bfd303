// Host-only check of RGB-D odometry (tests/test_odometry_host.py): csrc/icp_odometry.hip compiled by g++ against the HIP
// stand-in header (tests/hip_stub), built with -ffp-contract=off -fsanitize=address,undefined as a stand-alone program.
// The launchers are serial loops over the functions of csrc/icp_odometry_device.h -- the text the kernels compile --
// walking the block map, the blocks' pixels and the summation tree exactly as the kernels do.  "Device" buffers are host
// allocations of the size the host code asked for and every image of a case is an allocation that ends with its last
// row's last sample, so a record, an offset, a row stride or an output layout that is sized or addressed wrongly is an
// AddressSanitizer report.  Pyramids, traces, transformations, information matrices and counts are compared for equality
// with those of tests/odometry_reference.py, read from a text file (hexadecimal floats).
//   odometry_host_driver CASES.txt      exit code 0: every case equal and every refusal refused
//   odometry_host_driver --sincos X..   prints fdet_sincos_d of every argument as hexadecimal floats
// TEST INFRASTRUCTURE ONLY.
#include <functional>

#include "icp_host_prelude.h"
#include "../teaser-plusplus_amd/csrc/icp.hip"
#include "../teaser-plusplus_amd/csrc/icp_odometry.hip"

static int g_launches = 0;
static void expects(bool ok, const std::string& what, int c) { expect(ok, what.c_str(), c); }

namespace thip {

// fn(pair, pixel) for every thread of the launch over level l that is inside its pair's level, in block order
static void for_each_pixel(const OdoArgs& a, int l, const std::function<void(int, int32_t)>& fn) {
  ++g_launches;
  for (int blk = 0; blk < a.level_nblk[l]; ++blk) {
    const int p = a.blk_pair[a.level_blk0[l] + blk];
    if (p < 0 || p >= a.batch || blk < a.desc[p].blk_off[l]) std::abort();
    for (int t = 0; t < kOdoBlock; ++t) {
      const int32_t px = (blk - a.desc[p].blk_off[l]) * kOdoBlock + t;
      if (px < odo_n(a.desc[p], l)) fn(p, px);
    }
  }
}

static void host_match(const OdoArgs& a, int l) {
  for_each_pixel(a, l, [&](int p, int32_t s) {
    if (a.state[p].failed) return;
    int32_t pixel;
    uint64_t key;
    if (odo_px_match(a.desc[p], a.state[p], a.img, l, s, &pixel, &key)) {
      uint64_t* at = a.keys + a.desc[p].key_off + pixel;
      if (key < *at) *at = key;
    }
  });
}

static void host_sums_and_finish(const OdoArgs& a, int mode, int l, int next_level, int iter) {
  host_match(a, l);
  ++g_launches;
  for (int blk = 0; blk < a.level_nblk[l]; ++blk) {
    const int p = a.blk_pair[a.level_blk0[l] + blk];
    const OdoDesc& d = a.desc[p];
    if (a.state[p].failed) continue;
    static double v[kOdoBlock][kOdoSums];
    for (int t = 0; t < kOdoBlock; ++t) {
      const int32_t tp = (blk - d.blk_off[l]) * kOdoBlock + t;
      uint64_t key = kOdoEmptyKey;
      if (tp < odo_n(d, l)) {
        key = a.keys[d.key_off + tp];
        a.keys[d.key_off + tp] = kOdoEmptyKey;
      }
      odo_px_values(mode, d, a.state[p], a.img, l, tp, key, v[t]);
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
    const OdoDesc& d = a.desc[p];
    const bool failed = a.state[p].failed != 0;
    if (failed && mode != kOdoSumInfo) continue;
    double tot[kOdoSums];
    for (int k = 0; k < kOdoSums; ++k) tot[k] = failed ? 0.0 : odo_sum_blocks(a.part + d.part_off * kOdoSums, odo_blocks(d, l), k);
    teaser_icp_odometry_trace_c* rec = (mode == kOdoSumIter && d.trace_off >= 0) ? a.trace + d.trace_off + iter : nullptr;
    odo_finish(mode, d, a.state[p], tot, l, next_level, a.results + p, rec);
  }
}

void launch_odo_preprocess(hipStream_t, const OdoArgs& a, int levels, int next_level) {
  for_each_pixel(a, 0, [&](int p, int32_t px) {
    const OdoDesc& d = a.desc[p];
    odo_px_convert(d, a.in, a.tmp, 0, px / d.width, px % d.width);
    odo_px_convert(d, a.in, a.tmp, 1, px / d.width, px % d.width);
  });
  auto filter = [&](int l, int mode) {
    for_each_pixel(a, l, [&](int p, int32_t px) {
      const int w = odo_w(a.desc[p], l);
      odo_px_filter(a.desc[p], a.img, a.tmp, l, mode, px / w, px % w);
    });
  };
  filter(0, kOdoGaussIn);
  host_sums_and_finish(a, kOdoSumNorm, 0, next_level, 0);
  for_each_pixel(a, 0, [&](int p, int32_t px) {
    odo_px_scale_xyz(a.desc[p], a.state[p], a.img, px / a.desc[p].width, px % a.desc[p].width);
  });
  for (int l = 0; l + 1 < levels; ++l) {
    filter(l, kOdoGaussLevel);
    for_each_pixel(a, l + 1, [&](int p, int32_t px) {
      const int w = odo_w(a.desc[p], l + 1);
      odo_px_down(a.desc[p], a.img, a.tmp, l, px / w, px % w);
    });
  }
  for (int l = 0; l < levels; ++l) filter(l, kOdoSobel);
}

void launch_odo_iteration(hipStream_t, const OdoArgs& a, int level, int next_level, int iter) {
  host_sums_and_finish(a, kOdoSumIter, level, next_level, iter);
}

void launch_odo_information(hipStream_t, const OdoArgs& a) { host_sums_and_finish(a, kOdoSumInfo, 0, -1, 0); }

}  // namespace thip

// rows of `row` bytes, `pad` bytes of 0xAB between them, `comp` bytes per number: 2 uint16, 4 float32, 1 uint8
static void read_image(FILE* f, std::vector<unsigned char>& img, int64_t h, int64_t row, int64_t pad, int comp) {
  img.assign((size_t)((h - 1) * (row + pad) + row), 0xAB);
  for (int64_t i = 0; i < h; ++i)
    for (int64_t k = 0; k < row / comp; ++k) {
      const double v = read_number(f);
      unsigned char* at = img.data() + i * (row + pad) + k * comp;
      if (comp == 2) {
        const uint16_t s = (uint16_t)v;
        memcpy(at, &s, 2);
      } else if (comp == 4) {
        const float s = (float)v;
        memcpy(at, &s, 4);
      } else {
        *at = (unsigned char)v;
      }
    }
}

struct Case {
  teaser_icp_odometry_pair_c pair;
  teaser_icp_odometry_option_c opt;
  std::vector<unsigned char> img[4];
  std::vector<float> pyramid;
  teaser_icp_odometry_result_c res;
  std::vector<teaser_icp_odometry_trace_c> trace;
  int n_iter = 0;
};

static uint32_t bits32(float x) {
  uint32_t b;
  memcpy(&b, &x, 4);
  return b;
}
static bool same_doubles(const double* a, const double* b, size_t n) { return memcmp(a, b, 8 * n) == 0; }

static bool same_result(const teaser_icp_odometry_result_c& a, const teaser_icp_odometry_result_c& b) {
  return a.success == b.success && a.count == b.count && a.iterations == b.iterations && a.reserved == 0 &&
         same_doubles(a.transformation, b.transformation, 16) && same_doubles(a.information, b.information, 36);
}
static bool same_trace(const teaser_icp_odometry_trace_c& a, const teaser_icp_odometry_trace_c& b) {
  return a.level == b.level && a.executed == b.executed && a.count == b.count && a.failed == b.failed &&
         same_doubles(&a.e, &b.e, 1) && same_doubles(a.A, b.A, 21) && same_doubles(a.g, b.g, 6) && same_doubles(a.pose, b.pose, 16);
}

struct Batch {
  std::vector<teaser_icp_odometry_pair_c> pairs;
  std::vector<const void*> p[4];
  void add(const Case& cs) {
    pairs.push_back(cs.pair);
    for (int k = 0; k < 4; ++k) p[k].push_back(cs.img[k].data());
  }
};

static void refused(teaser_hip_icp* h, int32_t rc, const char* w1, const char* w2) {
  const std::string msg = h->err;
  expects(rc == TEASER_HIP_ERR_BAD_ARG && msg.find(w1) != std::string::npos && msg.find(w2) != std::string::npos,
         std::string("refusal: ") + w1 + " / " + msg, -1);
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::string(argv[1]) == "--sincos") {
    for (int k = 2; k < argc; ++k) {
      double s, c;
      thip::fdet_sincos_d(std::strtod(argv[k], nullptr), &s, &c);
      std::printf("%a %a\n", s, c);
    }
    return 0;
  }
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const int nc = (int)read_number(f);
  std::vector<Case> cases((size_t)nc);
  for (Case& cs : cases) {
    memset(&cs.pair, 0, sizeof(cs.pair));
    if (teaser_hip_icp_odometry_option_default(&cs.opt) != TEASER_HIP_OK) return 2;
    teaser_icp_odometry_pair_c& p = cs.pair;
    p.width = p.target_width = (int)read_number(f), p.height = p.target_height = (int)read_number(f);
    p.depth_format = (int)read_number(f), p.color_format = (int)read_number(f), p.jacobian = (int)read_number(f);
    const int64_t pad_d = (int64_t)read_number(f), pad_c = (int64_t)read_number(f);
    cs.opt.n_levels = (int)read_number(f);
    memset(cs.opt.iterations, 0, sizeof(cs.opt.iterations));
    for (int k = 0; k < cs.opt.n_levels; ++k) cs.n_iter += (cs.opt.iterations[k] = (int)read_number(f));
    p.fx = read_number(f), p.fy = read_number(f), p.cx = read_number(f), p.cy = read_number(f);
    for (double& m : p.odo_init) m = read_number(f);
    p.depth_scale = read_number(f), p.depth_trunc = read_number(f);
    cs.opt.depth_diff_max = read_number(f), cs.opt.depth_min = read_number(f), cs.opt.depth_max = read_number(f);
    const int dcomp = p.depth_format == 0 ? 2 : 4, ccomp = p.color_format == 1 ? 1 : 4;
    const int64_t drow = (int64_t)p.width * dcomp, crow = (int64_t)p.width * (p.color_format == 1 ? 3 : 4);
    p.source_depth_row_bytes = p.target_depth_row_bytes = drow + pad_d;
    p.source_color_row_bytes = p.target_color_row_bytes = crow + pad_c;
    for (int k = 0; k < 4; ++k) read_image(f, cs.img[k], p.height, k % 2 == 0 ? drow : crow, k % 2 == 0 ? pad_d : pad_c, k % 2 == 0 ? dcomp : ccomp);
    cs.pyramid.resize((size_t)(thip::kOdoPlanes * thip::odo_pyramid_pixels(p.width, p.height, cs.opt.n_levels)));
    for (float& x : cs.pyramid) x = (float)read_number(f);
    memset(&cs.res, 0, sizeof(cs.res));
    cs.res.success = (int)read_number(f), cs.res.count = (int)read_number(f), cs.res.iterations = (int)read_number(f);
    for (double& m : cs.res.transformation) m = read_number(f);
    for (double& m : cs.res.information) m = read_number(f);
    cs.trace.resize((size_t)cs.n_iter);
    for (teaser_icp_odometry_trace_c& t : cs.trace) {
      memset(&t, 0, sizeof(t));
      t.level = (int)read_number(f), t.executed = (int)read_number(f), t.count = (int)read_number(f), t.failed = (int)read_number(f);
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
    expects(teaser_hip_icp_rgbd_odometry_pyramid_batch(h, 1, one.pairs.data(), &cs.opt, one.p[0].data(), one.p[1].data(), one.p[2].data(),
                                                      one.p[3].data(), &out) == TEASER_HIP_OK, "pyramid: " + h->err, c);
    size_t diff = 0, first = 0;
    for (size_t k = 0; k < cs.pyramid.size(); ++k)
      if (bits32(pyr[k]) != bits32(cs.pyramid[k]) && diff++ == 0) first = k;
    expects(diff == 0, "pyramid bits: " + std::to_string(diff) + " differ, the first at float " + std::to_string(first), c);
    expects(pyr.back() == -7.5f, "a float behind the pyramid is written", c);
    teaser_icp_odometry_result_c res;
    memset(&res, 0xCD, sizeof(res));
    std::vector<teaser_icp_odometry_trace_c> tr((size_t)cs.n_iter + 1);
    memset(tr.data(), 0xCD, sizeof(tr[0]) * tr.size());
    teaser_icp_odometry_trace_c* trp = tr.data();
    g_launches = 0;
    expects(teaser_hip_icp_rgbd_odometry_batch(h, 1, one.pairs.data(), &cs.opt, one.p[0].data(), one.p[1].data(), one.p[2].data(),
                                              one.p[3].data(), &res, &trp) == TEASER_HIP_OK, "odometry: " + h->err, c);
    // preprocessing 3 L + 4 (convert, smooth, match / sums / finish, scale and XYZ, two per level step, a Sobel per
    // level), three per iteration, three for the information matrix
    expects(g_launches == 3 * cs.opt.n_levels + 4 + 3 * cs.n_iter + 3, "the launch count follows from the options alone", c);
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
    std::vector<teaser_icp_odometry_result_c> res((size_t)b);
    std::vector<std::vector<teaser_icp_odometry_trace_c>> tr((size_t)b, std::vector<teaser_icp_odometry_trace_c>((size_t)n_iter + 1));
    std::vector<teaser_icp_odometry_trace_c*> trp;
    for (int k = 0; k < b; ++k) trp.push_back(k % 2 == 0 ? tr[(size_t)k].data() : nullptr);
    expects(teaser_hip_icp_rgbd_odometry_batch(h, b, all.pairs.data(), &cases[(size_t)c0].opt, all.p[0].data(), all.p[1].data(),
                                              all.p[2].data(), all.p[3].data(), res.data(), trp.data()) == TEASER_HIP_OK, "batch: " + h->err, c0);
    std::vector<std::vector<float>> pyr;
    std::vector<float*> pp;
    for (int c : group) pyr.emplace_back(cases[(size_t)c].pyramid.size(), -7.5f);
    for (auto& v : pyr) pp.push_back(v.data());
    expects(teaser_hip_icp_rgbd_odometry_pyramid_batch(h, b, all.pairs.data(), &cases[(size_t)c0].opt, all.p[0].data(), all.p[1].data(),
                                                      all.p[2].data(), all.p[3].data(), pp.data()) == TEASER_HIP_OK, "pyramid batch: " + h->err, c0);
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
  teaser_icp_odometry_result_c res[2];
  auto call = [&](int which, void (*change)(teaser_icp_odometry_pair_c&), void (*change_opt)(teaser_icp_odometry_option_c&)) {
    std::vector<teaser_icp_odometry_pair_c> pr = two.pairs;
    teaser_icp_odometry_option_c o = c0.opt;
    if (change) change(pr[(size_t)which]);
    if (change_opt) change_opt(o);
    return teaser_hip_icp_rgbd_odometry_batch(h, 2, pr.data(), &o, two.p[0].data(), two.p[1].data(), two.p[2].data(), two.p[3].data(), res, nullptr);
  };
  typedef teaser_icp_odometry_pair_c PR;
  typedef teaser_icp_odometry_option_c OP;
  refused(h, call(1, [](PR& x) { x.depth_format = 2; }, nullptr), "depth_format", "pair 1");
  refused(h, call(0, [](PR& x) { x.color_format = 0; }, nullptr), "color_format", "pair 0");
  refused(h, call(0, [](PR& x) { x.color_format = 3; }, nullptr), "color_format", "pair 0");
  refused(h, call(1, [](PR& x) { x.jacobian = 2; }, nullptr), "jacobian", "pair 1");
  refused(h, call(1, [](PR& x) { x.reserved = 1; }, nullptr), "reserved", "pair 1");
  refused(h, call(0, [](PR& x) { x.target_width += 1; }, nullptr), "differ in size", "pair 0");
  refused(h, call(1, [](PR& x) { x.target_height -= 1; }, nullptr), "differ in size", "pair 1");
  refused(h, call(1, [](PR& x) { x.width = x.target_width = 3; }, nullptr), "every level needs a pixel", "pair 1");
  refused(h, call(0, [](PR& x) { x.height = x.target_height = 16385; }, nullptr), "width and height", "pair 0");
  refused(h, call(0, [](PR& x) { x.fx = 0.0; }, nullptr), "fx and fy", "pair 0");
  refused(h, call(1, [](PR& x) { x.fy = -1.0; }, nullptr), "fx and fy", "pair 1");
  refused(h, call(1, [](PR& x) { x.fx = NAN; }, nullptr), "fx and fy", "pair 1");
  refused(h, call(0, [](PR& x) { x.cy = INFINITY; }, nullptr), "cx and cy", "pair 0");
  refused(h, call(1, [](PR& x) { x.odo_init[6] = NAN; }, nullptr), "odo_init", "pair 1");
  refused(h, call(0, [](PR& x) { x.depth_scale = 0.0; }, nullptr), "depth_scale", "pair 0");
  refused(h, call(1, [](PR& x) { x.depth_trunc = NAN; }, nullptr), "depth_trunc", "pair 1");
  refused(h, call(1, [](PR& x) { x.source_depth_row_bytes = 1; }, nullptr), "source_depth_row_bytes", "pair 1");
  refused(h, call(0, [](PR& x) { x.target_color_row_bytes = 2; }, nullptr), "target_color_row_bytes", "pair 0");
  refused(h, call(0, nullptr, [](OP& o) { o.n_levels = 0; }), "n_levels", "");
  refused(h, call(0, nullptr, [](OP& o) { o.n_levels = 9; }), "n_levels", "");
  refused(h, call(0, nullptr, [](OP& o) { o.iterations[1] = -1; }), "iterations", "entry 1");
  refused(h, call(0, nullptr, [](OP& o) { o.reserved[2] = 1; }), "reserved", "option");
  refused(h, call(0, nullptr, [](OP& o) { o.depth_diff_max = NAN; }), "depth_diff_max", "");
  refused(h, call(0, nullptr, [](OP& o) { o.depth_min = INFINITY; }), "depth_min", "");
  refused(h, call(0, nullptr, [](OP& o) { o.depth_max = NAN; }), "depth_max", "");
  const void* half[2] = {c0.img[2].data(), nullptr};
  refused(h, teaser_hip_icp_rgbd_odometry_batch(h, 2, two.pairs.data(), &c0.opt, two.p[0].data(), two.p[1].data(), half, two.p[3].data(), res, nullptr),
          "target_depth is NULL", "pair 1");
  refused(h, teaser_hip_icp_rgbd_odometry_batch(h, 2, two.pairs.data(), &c0.opt, two.p[0].data(), nullptr, two.p[2].data(), two.p[3].data(), res, nullptr),
          "source_color must not be NULL", "");
  refused(h, teaser_hip_icp_rgbd_odometry_batch(h, 2, nullptr, &c0.opt, two.p[0].data(), two.p[1].data(), two.p[2].data(), two.p[3].data(), res, nullptr),
          "pairs must not be NULL", "");
  refused(h, teaser_hip_icp_rgbd_odometry_batch(h, 2, two.pairs.data(), nullptr, two.p[0].data(), two.p[1].data(), two.p[2].data(), two.p[3].data(), res, nullptr),
          "option must not be NULL", "");
  refused(h, teaser_hip_icp_rgbd_odometry_batch(h, 2, two.pairs.data(), &c0.opt, two.p[0].data(), two.p[1].data(), two.p[2].data(), two.p[3].data(), nullptr, nullptr),
          "results must not be NULL", "");
  refused(h, teaser_hip_icp_rgbd_odometry_batch(h, -1, two.pairs.data(), &c0.opt, two.p[0].data(), two.p[1].data(), two.p[2].data(), two.p[3].data(), res, nullptr),
          "batch", "");
  refused(h, teaser_hip_icp_rgbd_odometry_pyramid_batch(h, 2, two.pairs.data(), &c0.opt, two.p[0].data(), two.p[1].data(), two.p[2].data(), two.p[3].data(), nullptr),
          "images_out must not be NULL", "");
  expects(teaser_hip_icp_rgbd_odometry_batch(nullptr, 2, two.pairs.data(), &c0.opt, two.p[0].data(), two.p[1].data(), two.p[2].data(), two.p[3].data(), res, nullptr) ==
                 TEASER_HIP_ERR_BAD_ARG && teaser_hip_icp_odometry_option_default(nullptr) == TEASER_HIP_ERR_BAD_ARG, "refusal: NULL handle", -1);
  g_launches = 0;
  expects(teaser_hip_icp_rgbd_odometry_batch(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_OK &&
             teaser_hip_icp_rgbd_odometry_pyramid_batch(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_OK && g_launches == 0,
         "an empty batch does nothing", -1);
  teaser_icp_odometry_option_c d;
  expects(teaser_hip_icp_odometry_option_default(&d) == TEASER_HIP_OK && d.n_levels == 3 && d.iterations[0] == 20 && d.iterations[1] == 10 &&
             d.iterations[2] == 5 && d.iterations[3] == 0 && d.depth_diff_max == 0.03 && d.depth_min == 0.0 && d.depth_max == 4.0 && d.reserved2 == 0.0,
         "defaults", -1);
  // the handle works afterwards
  expects(teaser_hip_icp_rgbd_odometry_batch(h, 2, two.pairs.data(), &c0.opt, two.p[0].data(), two.p[1].data(), two.p[2].data(), two.p[3].data(), res, nullptr) ==
                 TEASER_HIP_OK && same_result(res[0], c0.res) && same_result(res[1], c0.res), "the handle works after the refusals", -1);
  teaser_hip_icp_destroy(h);
  std::printf("cases %d  mismatches %d\n", nc, g_bad);
  return g_bad ? 1 : 0;
}
