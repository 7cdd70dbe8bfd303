// Host-only check of the depth-frame calls (tests/test_rgbd_host.py): csrc/icp_rgbd.hip with icp.hip (the handle),
// compiled by g++ against the HIP stand-in header (tests/hip_stub), built with -ffp-contract=off
// -fsanitize=address,undefined.  The two launchers are serial loops over the functions of csrc/icp_rgbd_device.h -- the
// text the kernels compile -- walking the tile and block maps exactly as the kernels do: a count pass, the scan and a
// write pass that ranks the rows inside a tile; a serial minimum in place of the atomic one.  "Device" buffers are host
// allocations of the size the host code asked for and every image of a case is an allocation that ends with its last
// row's last sample, so a descriptor, an offset, a row stride or an output layout that is sized or addressed wrongly is
// an AddressSanitizer report.  Points, colours, pixels, counts, depth, colour and index images are compared for equality
// with those of tests/rgbd_reference.py, read from a text file (hexadecimal floats).
//   rgbd_host_driver CASES.txt    exit code 0: every case equal and every refusal refused
// TEST INFRASTRUCTURE ONLY.
#include "icp_host_prelude.h"
#include "../teaser-plusplus_amd/csrc/icp.hip"
#include "../teaser-plusplus_amd/csrc/icp_rgbd.hip"

namespace thip {

void launch_icp_rgbd_unproject(hipStream_t, const IcpFrameDesc* frames, const int32_t* tile_frame, int n_tiles, int batch,
                               const unsigned char* in, int32_t* tile_count, int32_t* tile_start, int32_t* count,
                               double* points, double* colors, int32_t* pixels) {
  auto visit = [&](const IcpFrameDesc& f, int tile, int t, int* i, int* j, int* ri, float* zf) {
    const int v = tile * kRgbdTile + t;
    if (v >= f.n_vis) return false;
    *ri = v / f.nj;
    *i = *ri * f.stride;
    *j = (v - *ri * f.nj) * f.stride;
    *zf = rgbd_depth(f, in + f.depth_off + (int64_t)*ri * f.width * rgbd_depth_bytes(f.depth_format), *j);
    return true;
  };
  for (int blk = 0; blk < n_tiles; ++blk) {
    const IcpFrameDesc& f = frames[tile_frame[blk]];
    if (blk < f.tile_off || blk >= f.tile_off + f.n_tiles) std::abort();  // a tile outside its frame
    int rows = 0, i, j, ri;
    float zf;
    for (int t = 0; t < kRgbdTile; ++t)
      if (visit(f, blk - f.tile_off, t, &i, &j, &ri, &zf) && (f.valid_only == 0 || rgbd_valid(zf))) ++rows;
    tile_count[blk] = rows;
  }
  for (int b = 0; b < batch; ++b) {
    int32_t run = 0;
    for (int k = 0; k < frames[b].n_tiles; ++k) {
      tile_start[frames[b].tile_off + k] = run;
      run += tile_count[frames[b].tile_off + k];
    }
    count[b] = run;
  }
  for (int blk = 0; blk < n_tiles; ++blk) {
    const IcpFrameDesc& f = frames[tile_frame[blk]];
    int rank = tile_start[blk], i, j, ri;
    float zf;
    for (int t = 0; t < kRgbdTile; ++t) {
      if (!visit(f, blk - f.tile_off, t, &i, &j, &ri, &zf)) continue;
      const bool valid = rgbd_valid(zf);
      if (f.valid_only != 0 && !valid) continue;
      double* p = points + 3 * (f.point_off + rank);
      if (valid) {
        rgbd_point(f, i, j, zf, p);
      } else {
        p[0] = p[1] = p[2] = NAN;
      }
      if (f.color_out >= 0)
        rgbd_color(f, in + f.color_off + (int64_t)ri * f.width * rgbd_color_bytes(f.color_format), j,
                   colors + 3 * (f.color_out + rank));
      if (f.pixel_out >= 0) pixels[f.pixel_out + rank] = i * f.width + j;
      ++rank;
    }
  }
}

void launch_icp_rgbd_project(hipStream_t, const IcpProjDesc* desc, const int32_t* blk_prob, int n_blk,
                             const int32_t* tile_prob, int n_tiles, const double* points, const double* colors,
                             uint64_t* keys, float* depth, float* color_img, int32_t* index_img, int32_t* n_hit) {
  for (int blk = 0; blk < n_blk; ++blk) {
    const IcpProjDesc& d = desc[blk_prob[blk]];
    for (int t = 0; t < kRgbdTile; ++t) {
      const int k = (blk - d.blk_off) * kRgbdTile + t;
      if (k < 0) std::abort();
      if (k >= d.n) continue;
      int32_t pixel;
      uint64_t key;
      if (!rgbd_project(d, points + 3 * (d.p_off + k), k, &pixel, &key)) continue;
      if (pixel < 0 || pixel >= d.width * d.height) std::abort();
      keys[d.img_off + pixel] = std::min(keys[d.img_off + pixel], key);
    }
  }
  for (int blk = 0; blk < n_tiles; ++blk) {
    const int b = tile_prob[blk];
    const IcpProjDesc& d = desc[b];
    for (int t = 0; t < kRgbdTile; ++t) {
      const int64_t px = (int64_t)(blk - d.tile_off) * kRgbdTile + t;
      if (px < 0) std::abort();
      if (px >= (int64_t)d.width * d.height) continue;
      float z;
      int32_t k;
      const bool hit = rgbd_resolve(keys[d.img_off + px], &z, &k);
      depth[d.img_off + px] = z;
      if (d.index_out >= 0) index_img[d.index_out + px] = k;
      if (d.color_out >= 0)
        for (int c = 0; c < 3; ++c) color_img[3 * (d.color_out + px) + c] = hit ? (float)colors[3 * (d.p_off + k) + c] : 0.0f;
      if (hit) n_hit[b] += 1;
    }
  }
}

}  // namespace thip

struct UCase {
  teaser_icp_frame_c f;
  std::vector<unsigned char> depth, color;  // as the caller holds them: padded rows, the last row cut after its samples
  int64_t n_vis = 0;
  int count = 0;
  std::vector<double> pts, col;
  std::vector<int32_t> pix;
};
struct PCase {
  teaser_icp_projection_c cam;
  int n = 0, has_color = 0, n_hit = 0;
  std::vector<double> pts, col;
  std::vector<float> depth, cimg;
  std::vector<int32_t> index;
};

// rows of `row` bytes, `pad` bytes of 0xAB between them, `comp` bytes per number: 2 uint16, 4 float32, 1 uint8
static void read_image(FILE* f, std::vector<unsigned char>& img, int64_t h, int64_t row, int64_t pad, int comp) {
  img.assign(h > 0 && row > 0 ? (size_t)((h - 1) * (row + pad) + row) : 0, 0xAB);
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

static bool same_f(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), 4 * a.size()) == 0);
}

static void refused(teaser_hip_icp* h, int32_t rc, const char* w1, const char* w2) {
  const std::string msg = teaser_hip_icp_last_error(h);
  expect(rc == TEASER_HIP_ERR_BAD_ARG && msg.find(w1) != std::string::npos && msg.find(w2) != std::string::npos,
         (std::string("refusal: ") + w1 + " / " + msg).c_str(), -1);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const int nu = (int)read_number(f), np = (int)read_number(f);
  std::vector<UCase> us((size_t)nu);
  std::vector<PCase> ps((size_t)np);
  for (UCase& c : us) {
    if (teaser_hip_icp_frame_default(&c.f) != TEASER_HIP_OK) return 2;
    c.f.width = (int)read_number(f), c.f.height = (int)read_number(f);
    c.f.depth_format = (int)read_number(f), c.f.color_format = (int)read_number(f);
    c.f.intensity = (int)read_number(f), c.f.stride = (int)read_number(f), c.f.valid_only = (int)read_number(f);
    const int64_t pad_d = (int64_t)read_number(f), pad_c = (int64_t)read_number(f);
    c.f.fx = read_number(f), c.f.fy = read_number(f), c.f.cx = read_number(f), c.f.cy = read_number(f);
    for (double& m : c.f.camera_pose) m = read_number(f);
    c.f.depth_scale = read_number(f), c.f.depth_trunc = read_number(f);
    const int dcomp = c.f.depth_format == 0 ? 2 : 4, ccomp = c.f.color_format == 1 ? 1 : 4;
    const int channels = c.f.color_format == 0 ? 0 : (c.f.color_format == 2 ? 1 : 3);
    const int64_t drow = (int64_t)c.f.width * dcomp, crow = (int64_t)c.f.width * channels * ccomp;
    c.f.depth_row_bytes = drow + pad_d, c.f.color_row_bytes = crow + pad_c;
    read_image(f, c.depth, c.f.height, drow, pad_d, dcomp);
    read_image(f, c.color, c.f.height, crow, pad_c, ccomp);
    c.n_vis = (int64_t)((c.f.height + c.f.stride - 1) / c.f.stride) * ((c.f.width + c.f.stride - 1) / c.f.stride);
    c.count = (int)read_number(f);
    read_numbers(f, c.pts, 3 * (size_t)c.count);
    if (c.f.color_format) read_numbers(f, c.col, 3 * (size_t)c.count);
    read_numbers(f, c.pix, (size_t)c.count);
  }
  for (PCase& c : ps) {
    memset(&c.cam, 0, sizeof(c.cam));
    c.n = (int)read_number(f), c.has_color = (int)read_number(f);
    c.cam.width = (int)read_number(f), c.cam.height = (int)read_number(f);
    c.cam.fx = read_number(f), c.cam.fy = read_number(f), c.cam.cx = read_number(f), c.cam.cy = read_number(f);
    for (double& m : c.cam.extrinsic) m = read_number(f);
    c.cam.depth_scale = read_number(f), c.cam.depth_max = read_number(f);
    read_numbers(f, c.pts, 3 * (size_t)c.n);
    if (c.has_color) read_numbers(f, c.col, 3 * (size_t)c.n);
    const size_t px = (size_t)c.cam.width * (size_t)c.cam.height;
    c.n_hit = (int)read_number(f);
    read_numbers(f, c.depth, px);
    read_numbers(f, c.index, px);
    if (c.has_color) read_numbers(f, c.cimg, 3 * px);
  }
  std::fclose(f);

  teaser_hip_icp* h = nullptr;
  if (teaser_hip_icp_create(0, &h) != TEASER_HIP_OK) return 2;

  // pass 0: every case alone; 1: all of them in one batch; 2: the batch reversed, some optional outputs left out
  for (int pass = 0; pass < 3; ++pass)
    for (int lo = 0; lo < nu; lo += pass ? nu : 1) {
      const int b = pass ? nu : 1;
      auto which = [&](int c) { return pass == 2 ? nu - 1 - c : lo + c; };
      std::vector<teaser_icp_frame_c> fr((size_t)b);
      std::vector<const void*> pd((size_t)b), pc((size_t)b);
      std::vector<int32_t> cnt((size_t)b, -5);
      std::vector<std::vector<double>> po((size_t)b), co((size_t)b);
      std::vector<std::vector<int32_t>> xo((size_t)b);
      std::vector<double*> ppo((size_t)b), pco((size_t)b);
      std::vector<int32_t*> pxo((size_t)b);
      for (int c = 0; c < b; ++c) {
        const UCase& cs = us[(size_t)which(c)];
        fr[c] = cs.f;
        pd[c] = cs.depth.empty() ? nullptr : cs.depth.data();
        pc[c] = cs.color.empty() ? nullptr : cs.color.data();
        po[c].assign(3 * (size_t)cs.n_vis, -7.5), co[c].assign(3 * (size_t)cs.n_vis, -7.5), xo[c].assign((size_t)cs.n_vis, -7);
        ppo[c] = cs.n_vis ? po[c].data() : nullptr;
        pco[c] = cs.n_vis && cs.f.color_format && (pass != 2 || c % 2 == 0) ? co[c].data() : nullptr;
        pxo[c] = cs.n_vis && (pass != 2 || c % 3 != 1) ? xo[c].data() : nullptr;
      }
      expect(teaser_hip_icp_unproject_depth_batch(h, b, fr.data(), pd.data(), pc.data(), cnt.data(), ppo.data(),
                                                  pco.data(), pxo.data()) == TEASER_HIP_OK,
             teaser_hip_icp_last_error(h), lo);
      for (int c = 0; c < b; ++c) {
        const UCase& cs = us[(size_t)which(c)];
        expect(cnt[c] == cs.count, "count", which(c));
        if (cnt[c] != cs.count) continue;
        const size_t m = (size_t)cs.count;
        expect(same(std::vector<double>(po[c].begin(), po[c].begin() + 3 * m), cs.pts), "point bits", which(c));
        for (size_t k = 3 * m; k < po[c].size(); ++k) expect(po[c][k] == -7.5, "a row behind the count is written", which(c));
        if (pco[c]) expect(same(std::vector<double>(co[c].begin(), co[c].begin() + 3 * m), cs.col), "colour bits", which(c));
        if (pxo[c]) expect(std::vector<int32_t>(xo[c].begin(), xo[c].begin() + m) == cs.pix, "pixels", which(c));
      }
    }
  for (int pass = 0; pass < 3; ++pass)
    for (int lo = 0; lo < np; lo += pass ? np : 1) {
      const int b = pass ? np : 1;
      auto which = [&](int c) { return pass == 2 ? np - 1 - c : lo + c; };
      std::vector<teaser_icp_projection_c> cam((size_t)b);
      std::vector<const double*> pp((size_t)b), pc((size_t)b);
      std::vector<int32_t> n((size_t)b), hit((size_t)b, -5);
      std::vector<std::vector<float>> dep((size_t)b), cim((size_t)b);
      std::vector<std::vector<int32_t>> idx((size_t)b);
      std::vector<float*> pdep((size_t)b), pcim((size_t)b);
      std::vector<int32_t*> pidx((size_t)b);
      for (int c = 0; c < b; ++c) {
        const PCase& cs = ps[(size_t)which(c)];
        const size_t px = (size_t)cs.cam.width * (size_t)cs.cam.height;
        cam[c] = cs.cam;
        pp[c] = cs.n ? cs.pts.data() : nullptr;
        pc[c] = cs.has_color ? cs.col.data() : nullptr;
        n[c] = cs.n;
        dep[c].assign(px, -7.5f), cim[c].assign(3 * px, -7.5f), idx[c].assign(px, -7);
        pdep[c] = px ? dep[c].data() : nullptr;
        pcim[c] = px && cs.has_color && (pass != 2 || c % 2 == 0) ? cim[c].data() : nullptr;
        pidx[c] = px && (pass != 2 || c % 3 != 1) ? idx[c].data() : nullptr;
      }
      expect(teaser_hip_icp_project_depth_batch(h, b, pp.data(), pc.data(), n.data(), cam.data(), pdep.data(), pcim.data(),
                                                pidx.data(), hit.data()) == TEASER_HIP_OK,
             teaser_hip_icp_last_error(h), lo);
      for (int c = 0; c < b; ++c) {
        const PCase& cs = ps[(size_t)which(c)];
        expect(hit[c] == cs.n_hit, "n_hit", which(c));
        expect(same_f(dep[c], cs.depth), "depth bits", which(c));
        if (pcim[c]) expect(same_f(cim[c], cs.cimg), "colour image bits", which(c));
        if (pidx[c]) expect(idx[c] == cs.index, "index image", which(c));
      }
    }

  // refusals: BAD_ARG, the argument and the problem named, and the handle still works
  {
    const UCase* pu = nullptr;
    for (const UCase& c : us)
      if (c.f.color_format == 1 && c.n_vis >= 30 && !pu) pu = &c;
    if (!pu) return 2;
    const UCase& cs = *pu;
    const void* pd[2] = {cs.depth.data(), cs.depth.data()};
    const void* pc[2] = {cs.color.data(), cs.color.data()};
    const void* half[2] = {cs.depth.data(), nullptr};
    std::vector<double> o0(3 * (size_t)cs.n_vis), o1(3 * (size_t)cs.n_vis), c0(3 * (size_t)cs.n_vis);
    double* po[2] = {o0.data(), o1.data()};
    double* po_half[2] = {nullptr, o1.data()};
    double* pco[2] = {c0.data(), nullptr};
    int32_t cnt[2];
    auto call = [&](int which, void (*change)(teaser_icp_frame_c&), double* const* colors_out = nullptr) {
      teaser_icp_frame_c fr[2] = {cs.f, cs.f};
      change(fr[which]);
      return teaser_hip_icp_unproject_depth_batch(h, 2, fr, pd, pc, cnt, po, colors_out, nullptr);
    };
    refused(h, call(1, [](teaser_icp_frame_c& x) { x.depth_format = 2; }), "depth_format", "problem 1");
    refused(h, call(0, [](teaser_icp_frame_c& x) { x.color_format = 4; }), "color_format", "problem 0");
    refused(h, call(1, [](teaser_icp_frame_c& x) { x.color_format = -1; }), "color_format", "problem 1");
    refused(h, call(0, [](teaser_icp_frame_c& x) { x.intensity = 2; }), "intensity", "problem 0");
    refused(h, call(1, [](teaser_icp_frame_c& x) { x.color_format = 0, x.intensity = 1; }), "intensity", "problem 1");
    refused(h, call(1, [](teaser_icp_frame_c& x) { x.valid_only = 2; }), "valid_only", "problem 1");
    refused(h, call(0, [](teaser_icp_frame_c& x) { x.reserved = 1; }), "reserved", "problem 0");
    refused(h, call(1, [](teaser_icp_frame_c& x) { x.stride = 0; }), "stride", "problem 1");
    refused(h, call(0, [](teaser_icp_frame_c& x) { x.fx = 0.0; }), "fx and fy", "problem 0");
    refused(h, call(1, [](teaser_icp_frame_c& x) { x.fy = NAN; }), "fx and fy", "problem 1");
    refused(h, call(1, [](teaser_icp_frame_c& x) { x.fx = INFINITY; }), "fx and fy", "problem 1");
    refused(h, call(0, [](teaser_icp_frame_c& x) { x.cx = INFINITY; }), "cx and cy", "problem 0");
    refused(h, call(1, [](teaser_icp_frame_c& x) { x.cy = NAN; }), "cx and cy", "problem 1");
    refused(h, call(1, [](teaser_icp_frame_c& x) { x.camera_pose[7] = NAN; }), "camera_pose", "problem 1");
    refused(h, call(0, [](teaser_icp_frame_c& x) { x.camera_pose[15] = INFINITY; }), "camera_pose", "problem 0");
    refused(h, call(0, [](teaser_icp_frame_c& x) { x.depth_scale = 0.0; }), "depth_scale", "problem 0");
    refused(h, call(1, [](teaser_icp_frame_c& x) { x.depth_scale = -1000.0; }), "depth_scale", "problem 1");
    refused(h, call(1, [](teaser_icp_frame_c& x) { x.depth_scale = INFINITY; }), "depth_scale", "problem 1");
    refused(h, call(0, [](teaser_icp_frame_c& x) { x.depth_trunc = NAN; }), "depth_trunc", "problem 0");
    refused(h, call(1, [](teaser_icp_frame_c& x) { x.depth_row_bytes = 2 * x.width - 1; }), "depth_row_bytes", "problem 1");
    refused(h, call(0, [](teaser_icp_frame_c& x) { x.color_row_bytes = 3 * x.width - 1; }), "color_row_bytes", "problem 0");
    refused(h, call(1, [](teaser_icp_frame_c& x) { x.width = 16385; }), "width and height", "problem 1");
    refused(h, call(0, [](teaser_icp_frame_c& x) { x.height = -1; }), "width and height", "problem 0");
    refused(h, call(0, [](teaser_icp_frame_c& x) { x.color_format = 0; }, pco), "without colour", "problem 0");
    {
      teaser_icp_frame_c fr[2] = {cs.f, cs.f};
      refused(h, teaser_hip_icp_unproject_depth_batch(h, 2, fr, half, pc, cnt, po, nullptr, nullptr), "depth is NULL", "problem 1");
      refused(h, teaser_hip_icp_unproject_depth_batch(h, 2, fr, pd, nullptr, cnt, po, nullptr, nullptr), "color is NULL", "problem 0");
      refused(h, teaser_hip_icp_unproject_depth_batch(h, 2, fr, pd, pc, cnt, po_half, nullptr, nullptr), "points_out is NULL", "problem 0");
      refused(h, teaser_hip_icp_unproject_depth_batch(h, 2, fr, pd, pc, cnt, nullptr, nullptr, nullptr), "points_out is NULL", "problem 0");
      refused(h, teaser_hip_icp_unproject_depth_batch(h, 2, nullptr, pd, pc, cnt, po, nullptr, nullptr), "frames must not be NULL", "");
      refused(h, teaser_hip_icp_unproject_depth_batch(h, 2, fr, pd, pc, nullptr, po, nullptr, nullptr), "count_out must not be NULL", "");
      expect(teaser_hip_icp_unproject_depth_batch(h, -1, fr, pd, pc, cnt, po, nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG, "refusal: batch", -1);
      expect(teaser_hip_icp_unproject_depth_batch(nullptr, 2, fr, pd, pc, cnt, po, nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG, "refusal: handle", -1);
      expect(teaser_hip_icp_unproject_depth_batch(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_OK, "an empty batch", -1);
      // 2^31 - 1 visited pixels: eight frames of 16384 x 16384 hold 2^31; the sizes are checked before any pointer of a
      // later frame, so the images need not exist
      std::vector<teaser_icp_frame_c> big(8, cs.f);
      std::vector<const void*> bd(8, cs.depth.data()), bc(8, cs.color.data());
      std::vector<double*> bo(8, o0.data());
      std::vector<int32_t> bcnt(8);
      for (teaser_icp_frame_c& x : big) x.width = x.height = 16384, x.depth_row_bytes = 2 * 16384, x.color_row_bytes = 3 * 16384;
      refused(h, teaser_hip_icp_unproject_depth_batch(h, 8, big.data(), bd.data(), bc.data(), bcnt.data(), bo.data(), nullptr, nullptr),
              "2^31 - 1 visited pixels", "");
      // frames without pixels need no pointer at all
      teaser_icp_frame_c none[2] = {cs.f, cs.f};
      none[0].width = 0, none[1].height = 0;
      cnt[0] = cnt[1] = -3;
      expect(teaser_hip_icp_unproject_depth_batch(h, 2, none, nullptr, nullptr, cnt, nullptr, nullptr, nullptr) == TEASER_HIP_OK &&
                 cnt[0] == 0 && cnt[1] == 0, "a batch of empty frames", -1);
      expect(teaser_hip_icp_unproject_depth_batch(h, 2, fr, pd, pc, cnt, po, pco, nullptr) == TEASER_HIP_OK && cnt[0] == cs.count &&
                 cnt[1] == cs.count, "the handle works afterwards", -1);
      o0.resize(3 * (size_t)cs.count), o1.resize(3 * (size_t)cs.count), c0.resize(3 * (size_t)cs.count);
      expect(same(o0, cs.pts) && same(o1, cs.pts) && same(c0, cs.col), "two copies of a frame agree with the restatement", -1);
    }

    const PCase* pp = nullptr;
    for (const PCase& c : ps)
      if (c.has_color && c.n >= 30 && c.cam.width * c.cam.height >= 6 && !pp) pp = &c;
    if (!pp) return 2;
    const PCase& pj = *pp;
    const size_t px = (size_t)pj.cam.width * (size_t)pj.cam.height;
    const double* pts[2] = {pj.pts.data(), pj.pts.data()};
    const double* col[2] = {pj.col.data(), pj.col.data()};
    std::vector<double> bad_p = pj.pts, bad_c = pj.col;
    bad_p[4] = NAN, bad_c[7] = INFINITY;
    const double* pts_bad[2] = {pj.pts.data(), bad_p.data()};
    const double* col_bad[2] = {bad_c.data(), pj.col.data()};
    const int32_t n[2] = {pj.n, pj.n}, n_neg[2] = {pj.n, -1};
    std::vector<float> d0(px), d1(px), ci(3 * px);
    float* pdep[2] = {d0.data(), d1.data()};
    float* pdep_half[2] = {d0.data(), nullptr};
    float* pci[2] = {nullptr, ci.data()};
    int32_t hit[2];
    auto pcall = [&](int which, void (*change)(teaser_icp_projection_c&)) {
      teaser_icp_projection_c cam[2] = {pj.cam, pj.cam};
      change(cam[which]);
      return teaser_hip_icp_project_depth_batch(h, 2, pts, col, n, cam, pdep, nullptr, nullptr, hit);
    };
    refused(h, pcall(1, [](teaser_icp_projection_c& x) { x.width = 16385; }), "width and height", "problem 1");
    refused(h, pcall(0, [](teaser_icp_projection_c& x) { x.height = -2; }), "width and height", "problem 0");
    refused(h, pcall(0, [](teaser_icp_projection_c& x) { x.fy = 0.0; }), "fx and fy", "problem 0");
    refused(h, pcall(1, [](teaser_icp_projection_c& x) { x.fx = NAN; }), "fx and fy", "problem 1");
    refused(h, pcall(1, [](teaser_icp_projection_c& x) { x.cx = NAN; }), "cx and cy", "problem 1");
    refused(h, pcall(0, [](teaser_icp_projection_c& x) { x.extrinsic[3] = INFINITY; }), "extrinsic", "problem 0");
    refused(h, pcall(1, [](teaser_icp_projection_c& x) { x.depth_scale = 0.0; }), "depth_scale", "problem 1");
    refused(h, pcall(0, [](teaser_icp_projection_c& x) { x.depth_scale = NAN; }), "depth_scale", "problem 0");
    refused(h, pcall(1, [](teaser_icp_projection_c& x) { x.depth_max = INFINITY; }), "depth_max", "problem 1");
    teaser_icp_projection_c cam[2] = {pj.cam, pj.cam};
    refused(h, teaser_hip_icp_project_depth_batch(h, 2, pts_bad, col, n, cam, pdep, nullptr, nullptr, hit), "points has a non-finite", "problem 1");
    refused(h, teaser_hip_icp_project_depth_batch(h, 2, pts, col_bad, n, cam, pdep, nullptr, nullptr, hit), "colors has a non-finite", "problem 0");
    refused(h, teaser_hip_icp_project_depth_batch(h, 2, pts, col, n_neg, cam, pdep, nullptr, nullptr, hit), "n must be", "problem 1");
    refused(h, teaser_hip_icp_project_depth_batch(h, 2, nullptr, col, n, cam, pdep, nullptr, nullptr, hit), "points is NULL", "problem 0");
    refused(h, teaser_hip_icp_project_depth_batch(h, 2, pts, col, n, cam, pdep_half, nullptr, nullptr, hit), "depth_out is NULL", "problem 1");
    refused(h, teaser_hip_icp_project_depth_batch(h, 2, pts, col, n, cam, nullptr, nullptr, nullptr, hit), "depth_out is NULL", "problem 0");
    refused(h, teaser_hip_icp_project_depth_batch(h, 2, pts, nullptr, n, cam, pdep, pci, nullptr, hit), "without colours", "problem 1");
    refused(h, teaser_hip_icp_project_depth_batch(h, 2, pts, col, n, nullptr, pdep, nullptr, nullptr, hit), "cameras must not be NULL", "");
    refused(h, teaser_hip_icp_project_depth_batch(h, 2, pts, col, n, cam, pdep, nullptr, nullptr, nullptr), "n_hit_out must not be NULL", "");
    refused(h, teaser_hip_icp_project_depth_batch(h, 2, pts, col, nullptr, cam, pdep, nullptr, nullptr, hit), "n must not be NULL", "");
    {
      std::vector<teaser_icp_projection_c> big(8, pj.cam);
      std::vector<const double*> bp(8, pj.pts.data());
      std::vector<int32_t> bn(8, pj.n), bh(8);
      std::vector<float*> bd(8, d0.data());
      for (teaser_icp_projection_c& x : big) x.width = x.height = 16384;
      refused(h, teaser_hip_icp_project_depth_batch(h, 8, bp.data(), nullptr, bn.data(), big.data(), bd.data(), nullptr, nullptr, bh.data()),
              "2^31 - 1 pixels", "");
    }
    expect(teaser_hip_icp_project_depth_batch(h, -1, pts, col, n, cam, pdep, nullptr, nullptr, hit) == TEASER_HIP_ERR_BAD_ARG, "refusal: batch", -1);
    expect(teaser_hip_icp_project_depth_batch(nullptr, 2, pts, col, n, cam, pdep, nullptr, nullptr, hit) == TEASER_HIP_ERR_BAD_ARG, "refusal: handle", -1);
    expect(teaser_hip_icp_project_depth_batch(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_OK,
           "an empty batch", -1);
    // images without points: empty images, and with no point in the whole call no device work at all
    const int32_t zero[2] = {0, 0};
    std::vector<int32_t> i0(px, 5);
    int32_t* pix[2] = {i0.data(), nullptr};
    d0.assign(px, 3.0f), d1.assign(px, 3.0f);
    hit[0] = hit[1] = -3;
    expect(teaser_hip_icp_project_depth_batch(h, 2, nullptr, nullptr, zero, cam, pdep, nullptr, pix, hit) == TEASER_HIP_OK && hit[0] == 0 &&
               hit[1] == 0 && d0 == std::vector<float>(px, 0.0f) && d1 == d0 && i0 == std::vector<int32_t>(px, -1),
           "a batch without points", -1);
    expect(teaser_hip_icp_project_depth_batch(h, 2, pts, col, n, cam, pdep, pci, pix, hit) == TEASER_HIP_OK && hit[0] == pj.n_hit &&
               hit[1] == pj.n_hit, "the handle works afterwards", -1);
    expect(same_f(d0, pj.depth) && same_f(d1, pj.depth) && same_f(ci, pj.cimg) && i0 == pj.index,
           "two copies of a cloud agree with the restatement", -1);
  }
  teaser_hip_icp_destroy(h);
  std::printf("cases %d  mismatches %d\n", nu + np, g_bad);
  return g_bad ? 1 : 0;
}
