// Host-only check of the TSDF volume (tests/test_tsdf_host.py): csrc/tsdf.hip compiled by g++ against the HIP stand-in
// header (tests/hip_stub), built with -ffp-contract=off -fsanitize=address,undefined as a stand-alone program.  The
// launchers are serial loops over the functions of csrc/tsdf_device.h -- the text the kernels compile -- walking columns,
// z segments, frames and rows exactly as the kernels do.  "Device" buffers are host allocations of the size the host code
// asked for and every image of a case is an allocation that ends with its last row's last sample, so a record, an
// offset, a row stride or an output layout that is sized or addressed wrongly is an AddressSanitizer report.  Voxels,
// counts, points, normals and colours are compared for equality with those of tests/tsdf_reference.py, read from a text
// file (hexadecimal floats).
//   tsdf_host_driver CASES.txt    exit code 0: every case equal and every refusal refused
// TEST INFRASTRUCTURE ONLY.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define __forceinline__ inline
#include "../teaser-plusplus_amd/csrc/tsdf.hip"

static int g_bad = 0, g_integrate_launches = 0, g_segments_seen = 0;
static void expect(bool ok, const char* what, int c) {
  if (!ok) {
    std::fprintf(stderr, "case %d: %s\n", c, what);
    ++g_bad;
  }
}

namespace thip {

void launch_tsdf_integrate(hipStream_t, const TsdfGrid& g, const TsdfChunkArgs& ck, const unsigned char* in,
                           const TsdfFields& v) {
  ++g_integrate_launches;
  g_segments_seen = ck.segments;
  if (ck.n < 1 || ck.n > kTsdfChunk || ck.segments < 1 || ck.segments > g.R) std::abort();
  const int64_t plane = (int64_t)g.R * g.R;
  const int seg_len = (g.R + ck.segments - 1) / ck.segments;
  for (int seg = 0; seg < ck.segments; ++seg)
    for (int64_t col = 0; col < plane; ++col) {
      const int x = (int)(col / g.R), y = (int)(col - (int64_t)x * g.R);
      const int z0 = seg * seg_len, z1 = std::min(z0 + seg_len, (int)g.R);
      float c[kTsdfChunk][3];
      for (int k = 0; k < ck.n; ++k) tsdf_column_start(g, ck.f[k], x, y, c[k]);
      for (int z = 0; z < z0; ++z)
        for (int k = 0; k < ck.n; ++k) tsdf_column_step(ck.f[k], c[k]);
      for (int z = z0; z < z1; ++z) {
        const int64_t at = (int64_t)z * plane + col;
        if (at != tsdf_index(g.R, x, y, z) || at >= v.n) std::abort();
        bool loaded = false;
        float tv = 0.0f, wv = 0.0f;
        double cv[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < ck.n; ++k) {
          float t;
          double s[3] = {0.0, 0.0, 0.0};
          if (tsdf_hit(g, ck.f[k], in, c[k], &t, s)) {
            if (!loaded) {
              loaded = true;
              tv = v.tsdf[at], wv = v.weight[at];
              if (g.color_type != 0)
                for (int q = 0; q < 3; ++q) cv[q] = v.color[q * v.n + at];
            }
            tsdf_update(g, t, s, &tv, &wv, cv);
          }
          tsdf_column_step(ck.f[k], c[k]);
        }
        if (loaded) {
          v.tsdf[at] = tv, v.weight[at] = wv;
          if (g.color_type != 0)
            for (int q = 0; q < 3; ++q) v.color[q * v.n + at] = cv[q];
        }
      }
    }
}

void launch_tsdf_count(hipStream_t, const TsdfGrid& g, const TsdfFields& v, int mode, int32_t* counts, int64_t* offsets) {
  const int64_t plane = (int64_t)g.R * g.R;
  int64_t run = 0;
  for (int64_t col = 0; col < plane; ++col) {
    const int x = (int)(col / g.R), y = (int)(col % g.R);
    int32_t rows = 0;
    for (int z = 0; z < g.R; ++z) rows += tsdf_voxel_rows(g, v, mode, x, y, z);
    counts[col] = rows;
    offsets[col] = run;
    run += rows;
  }
  offsets[plane] = run;
}

void launch_tsdf_write(hipStream_t, const TsdfGrid& g, const TsdfFields& v, int mode, const int64_t* offsets,
                       int64_t capacity, double* points, double* normals, double* colors) {
  const int64_t plane = (int64_t)g.R * g.R;
  if (offsets[plane] > capacity) return;
  for (int64_t col = 0; col < plane; ++col) {
    const int x = (int)(col / g.R), y = (int)(col % g.R);
    int64_t row = offsets[col];
    for (int z = 0; z < g.R; ++z) {
      const int64_t at0 = tsdf_index(g.R, x, y, z);
      const float f0 = v.tsdf[at0];
      if (!tsdf_usable(v.weight[at0], f0)) continue;
      if (mode == 1) {
        tsdf_voxel_point(g, x, y, z, f0, points + 3 * row, colors ? colors + 3 * row : nullptr);
        ++row;
        continue;
      }
      for (int i = 0; i < 3; ++i) {
        int64_t at1;
        float f1;
        if (!tsdf_surface_row(g, v, x, y, z, i, f0, &at1, &f1)) continue;
        tsdf_surface_point(g, v, x, y, z, i, f0, at1, f1, points + 3 * row, normals ? normals + 3 * row : nullptr,
                           colors ? colors + 3 * row : nullptr);
        ++row;
      }
    }
    if (row != offsets[col + 1]) std::abort();  // the write pass and the count pass disagree
  }
}

void launch_tsdf_export(hipStream_t, const TsdfGrid& g, const TsdfFields& v, float* tw, double* color) {
  for (int x = 0; x < g.R; ++x)
    for (int y = 0; y < g.R; ++y)
      for (int z = 0; z < g.R; ++z) {
        const int64_t at = tsdf_index(g.R, x, y, z), o = ((int64_t)x * g.R + y) * g.R + z;
        if (tw) tw[2 * o] = v.tsdf[at], tw[2 * o + 1] = v.weight[at];
        if (color)
          for (int k = 0; k < 3; ++k) color[3 * o + k] = v.color[k * v.n + at];
      }
}

void launch_tsdf_import(hipStream_t, const TsdfGrid& g, const TsdfFields& v, const float* tw, const double* color) {
  for (int x = 0; x < g.R; ++x)
    for (int y = 0; y < g.R; ++y)
      for (int z = 0; z < g.R; ++z) {
        const int64_t at = tsdf_index(g.R, x, y, z), o = ((int64_t)x * g.R + y) * g.R + z;
        if (tw) v.tsdf[at] = tw[2 * o], v.weight[at] = tw[2 * o + 1];
        if (color)
          for (int k = 0; k < 3; ++k) v.color[k * v.n + at] = rgbd_canonical(color[3 * o + k]);
      }
}

}  // namespace thip

// The next token of the case file as a number: decimal integers, hexadecimal floats, "nan", "inf".
static double read_number(FILE* f) {
  char tok[64];
  if (std::fscanf(f, "%63s", tok) != 1) std::exit(2);
  return std::strtod(tok, nullptr);
}
template <class T>
static void read_numbers(FILE* f, std::vector<T>& v, size_t cnt) {
  v.resize(cnt);
  for (T& x : v) x = (T)read_number(f);
}
template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0);
}

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

struct Frame {
  teaser_tsdf_frame_c f;
  std::vector<unsigned char> depth, color;
};
struct Case {
  teaser_tsdf_volume_c vol;
  std::vector<Frame> frames;
  std::vector<float> tw;
  std::vector<double> color, pts, nrm, col, vpts, vcol;
  int64_t count = 0, vcount = 0;
};

static void refused(teaser_hip_tsdf* h, int32_t rc, const char* w1, const char* w2) {
  const std::string msg = teaser_hip_tsdf_last_error(h);
  expect(rc == TEASER_HIP_ERR_BAD_ARG && msg.find(w1) != std::string::npos && msg.find(w2) != std::string::npos,
         (std::string("refusal: ") + w1 + " / " + msg).c_str(), -1);
}

static void refused_create(void (*change)(teaser_tsdf_volume_c&), const char* word) {
  teaser_tsdf_volume_c v;
  teaser_hip_tsdf_volume_default(&v);
  v.resolution = 4;
  change(v);
  teaser_hip_tsdf* h = (teaser_hip_tsdf*)16;
  const int32_t rc = teaser_hip_tsdf_create(&v, 0, &h);
  refused(nullptr, rc, word, "");
  expect(h == nullptr, "a refused create leaves *out NULL", -1);
}

static std::vector<const void*> ptrs(const std::vector<Frame>& fr, bool color) {
  std::vector<const void*> p;
  for (const Frame& x : fr) {
    const std::vector<unsigned char>& img = color ? x.color : x.depth;
    p.push_back(img.empty() ? nullptr : img.data());
  }
  return p;
}

// The whole state and both extractions of `h` against the case.
static void check_volume(teaser_hip_tsdf* h, const Case& cs, int c, const char* when) {
  const size_t n = (size_t)cs.vol.resolution * cs.vol.resolution * cs.vol.resolution;
  const bool colored = cs.vol.color_type != 0;
  const std::string tag = std::string(" (") + when + ")";
  std::vector<float> tw(2 * n, -7.5f);
  std::vector<double> color(colored ? 3 * n : 0, -7.5);
  expect(teaser_hip_tsdf_download(h, tw.data(), colored ? color.data() : nullptr) == TEASER_HIP_OK, "download", c);
  expect(same(tw, cs.tw), ("tsdf and weight bits" + tag).c_str(), c);
  if (colored) expect(same(color, cs.color), ("colour bits" + tag).c_str(), c);
  int64_t count = -5;
  expect(teaser_hip_tsdf_extract_point_cloud(h, 0, nullptr, nullptr, nullptr, &count) == TEASER_HIP_OK && count == cs.count,
         ("count" + tag).c_str(), c);
  if (count != cs.count) return;
  const size_t m = (size_t)count;
  std::vector<double> p(3 * m + 3, -7.5), nn(3 * m + 3, -7.5), cc(3 * m + 3, -7.5);
  count = -5;
  expect(teaser_hip_tsdf_extract_point_cloud(h, (int64_t)m, p.data(), nn.data(), colored ? cc.data() : nullptr, &count) == TEASER_HIP_OK &&
             count == cs.count, "extraction with the exact capacity", c);
  for (size_t k = 3 * m; k < 3 * m + 3; ++k)
    expect(p[k] == -7.5 && nn[k] == -7.5 && cc[k] == -7.5, "a row behind the count is written", c);
  p.resize(3 * m), nn.resize(3 * m), cc.resize(3 * m);
  expect(same(p, cs.pts), ("point bits" + tag).c_str(), c);
  expect(same(nn, cs.nrm), ("normal bits" + tag).c_str(), c);
  if (colored) expect(same(cc, cs.col), ("point colour bits" + tag).c_str(), c);
  if (m > 0) {  // one row too few: refused, the count named and reported, nothing written
    std::vector<double> q(3 * m, -7.5), qn(3 * m, -7.5);
    count = -5;
    refused(h, teaser_hip_tsdf_extract_point_cloud(h, (int64_t)m - 1, q.data(), qn.data(), nullptr, &count), "capacity",
            ("count " + std::to_string(m)).c_str());
    expect(count == cs.count, "the refused extraction reports the count", c);
    expect(q == std::vector<double>(3 * m, -7.5) && qn == q, "the refused extraction writes nothing", c);
    // generous room and no optional output
    std::vector<double> big(3 * (m + 100), -7.5);
    expect(teaser_hip_tsdf_extract_point_cloud(h, (int64_t)m + 100, big.data(), nullptr, nullptr, &count) == TEASER_HIP_OK,
           "extraction with room to spare", c);
    big.resize(3 * m);
    expect(same(big, cs.pts), "point bits with room to spare", c);
  }
  int64_t vcount = -5;
  expect(teaser_hip_tsdf_extract_voxel_point_cloud(h, 0, nullptr, nullptr, &vcount) == TEASER_HIP_OK && vcount == cs.vcount,
         ("voxel count" + tag).c_str(), c);
  if (vcount != cs.vcount) return;
  std::vector<double> vp(3 * (size_t)vcount, -7.5), vc(3 * (size_t)vcount, -7.5);
  expect(teaser_hip_tsdf_extract_voxel_point_cloud(h, vcount, vcount ? vp.data() : nullptr, vcount ? vc.data() : nullptr, &vcount) ==
             TEASER_HIP_OK, "voxel cloud", c);
  expect(same(vp, cs.vpts) && same(vc, cs.vcol), ("voxel cloud bits" + tag).c_str(), c);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const int nc = (int)read_number(f);
  std::vector<Case> cases((size_t)nc);
  for (Case& cs : cases) {
    if (teaser_hip_tsdf_volume_default(&cs.vol) != TEASER_HIP_OK) return 2;
    cs.vol.resolution = (int)read_number(f), cs.vol.color_type = (int)read_number(f);
    cs.frames.resize((size_t)read_number(f));
    cs.vol.length = read_number(f), cs.vol.sdf_trunc = read_number(f);
    for (double& o : cs.vol.origin) o = read_number(f);
    for (Frame& fr : cs.frames) {
      memset(&fr.f, 0, sizeof(fr.f));
      fr.f.width = (int)read_number(f), fr.f.height = (int)read_number(f);
      fr.f.depth_format = (int)read_number(f), fr.f.color_format = (int)read_number(f);
      const int64_t pad_d = (int64_t)read_number(f), pad_c = (int64_t)read_number(f);
      fr.f.fx = read_number(f), fr.f.fy = read_number(f), fr.f.cx = read_number(f), fr.f.cy = read_number(f);
      for (double& m : fr.f.extrinsic) m = read_number(f);
      fr.f.depth_scale = read_number(f), fr.f.depth_trunc = read_number(f);
      const int dcomp = fr.f.depth_format == 0 ? 2 : 4, ccomp = fr.f.color_format == 1 ? 1 : 4;
      const int channels = fr.f.color_format == 0 ? 0 : (fr.f.color_format == 2 ? 1 : 3);
      const int64_t drow = (int64_t)fr.f.width * dcomp, crow = (int64_t)fr.f.width * channels * ccomp;
      fr.f.depth_row_bytes = drow + pad_d, fr.f.color_row_bytes = crow + pad_c;
      read_image(f, fr.depth, fr.f.height, drow, pad_d, dcomp);
      read_image(f, fr.color, fr.f.height, crow, pad_c, ccomp);
    }
    const size_t n = (size_t)cs.vol.resolution * cs.vol.resolution * cs.vol.resolution;
    read_numbers(f, cs.tw, 2 * n);
    if (cs.vol.color_type) read_numbers(f, cs.color, 3 * n);
    cs.count = (int64_t)read_number(f);
    read_numbers(f, cs.pts, 3 * (size_t)cs.count);
    read_numbers(f, cs.nrm, 3 * (size_t)cs.count);
    if (cs.vol.color_type) read_numbers(f, cs.col, 3 * (size_t)cs.count);
    cs.vcount = (int64_t)read_number(f);
    read_numbers(f, cs.vpts, 3 * (size_t)cs.vcount);
    read_numbers(f, cs.vcol, 3 * (size_t)cs.vcount);
  }
  std::fclose(f);

  for (int c = 0; c < nc; ++c) {
    const Case& cs = cases[(size_t)c];
    const int nf = (int)cs.frames.size();
    const size_t n = (size_t)cs.vol.resolution * cs.vol.resolution * cs.vol.resolution;
    teaser_hip_tsdf *a = nullptr, *b = nullptr;  // two volumes alive at once
    if (teaser_hip_tsdf_create(&cs.vol, 0, &a) != TEASER_HIP_OK || teaser_hip_tsdf_create(&cs.vol, -1, &b) != TEASER_HIP_OK) return 2;
    std::vector<teaser_tsdf_frame_c> recs;
    for (const Frame& fr : cs.frames) recs.push_back(fr.f);
    const std::vector<const void*> pd = ptrs(cs.frames, false), pc = ptrs(cs.frames, true);
    // a: every frame in one call; b: one call per frame
    g_integrate_launches = 0;
    expect(teaser_hip_tsdf_integrate_batch(a, nf, recs.data(), pd.data(), pc.data()) == TEASER_HIP_OK, teaser_hip_tsdf_last_error(a), c);
    expect(g_integrate_launches == (nf + thip::kTsdfChunk - 1) / thip::kTsdfChunk, "one launch per chunk of frames", c);
    if (nf > 0) expect(g_segments_seen == thip::tsdf_segments(cs.vol.resolution), "the z segments of the launch", c);
    for (int k = 0; k < nf; ++k)
      expect(teaser_hip_tsdf_integrate_batch(b, 1, &recs[(size_t)k], &pd[(size_t)k], &pc[(size_t)k]) == TEASER_HIP_OK,
             teaser_hip_tsdf_last_error(b), c);
    check_volume(a, cs, c, "one call");
    check_volume(b, cs, c, "a call per frame");
    // reset, then the state back through upload
    expect(teaser_hip_tsdf_reset(b) == TEASER_HIP_OK, "reset", c);
    std::vector<float> tw(2 * n, -7.5f);
    expect(teaser_hip_tsdf_download(b, tw.data(), nullptr) == TEASER_HIP_OK && tw == std::vector<float>(2 * n, 0.0f), "reset leaves zeros", c);
    int64_t count = -5;
    expect(teaser_hip_tsdf_extract_point_cloud(b, 0, nullptr, nullptr, nullptr, &count) == TEASER_HIP_OK && count == 0, "an empty volume has no rows", c);
    expect(teaser_hip_tsdf_upload(b, cs.tw.data(), cs.vol.color_type ? cs.color.data() : nullptr) == TEASER_HIP_OK, "upload", c);
    check_volume(b, cs, c, "after reset and upload");
    teaser_hip_tsdf_destroy(a);
    teaser_hip_tsdf_destroy(b);
  }

  // refusals: BAD_ARG with the argument (and the frame) named; the handle stays usable
  refused_create([](teaser_tsdf_volume_c& v) { v.resolution = 0; }, "resolution");
  refused_create([](teaser_tsdf_volume_c& v) { v.resolution = 1025; }, "resolution");
  refused_create([](teaser_tsdf_volume_c& v) { v.length = 0.0; }, "length");
  refused_create([](teaser_tsdf_volume_c& v) { v.length = INFINITY; }, "length");
  refused_create([](teaser_tsdf_volume_c& v) { v.sdf_trunc = -0.1; }, "sdf_trunc");
  refused_create([](teaser_tsdf_volume_c& v) { v.sdf_trunc = NAN; }, "sdf_trunc");
  refused_create([](teaser_tsdf_volume_c& v) { v.origin[1] = NAN; }, "origin");
  refused_create([](teaser_tsdf_volume_c& v) { v.color_type = 3; }, "color_type");
  refused_create([](teaser_tsdf_volume_c& v) { v.color_type = -1; }, "color_type");
  refused_create([](teaser_tsdf_volume_c& v) { v.reserved = 1; }, "reserved");
  {
    teaser_hip_tsdf* h = nullptr;
    expect(teaser_hip_tsdf_create(nullptr, 0, &h) == TEASER_HIP_ERR_BAD_ARG && h == nullptr, "refusal: volume NULL", -1);
    expect(teaser_hip_tsdf_create(&cases[0].vol, 0, nullptr) == TEASER_HIP_ERR_BAD_ARG, "refusal: out NULL", -1);
    expect(teaser_hip_tsdf_volume_default(nullptr) == TEASER_HIP_ERR_BAD_ARG, "refusal: default NULL", -1);
    teaser_tsdf_volume_c d;
    expect(teaser_hip_tsdf_volume_default(&d) == TEASER_HIP_OK && d.length == 4.0 && d.sdf_trunc == 0.04 && d.resolution == 512 &&
               d.color_type == 0 && d.reserved == 0 && d.origin[0] == 0.0 && d.origin[2] == 0.0, "defaults", -1);
  }
  const Case* rgb = nullptr;
  const Case* gray = nullptr;
  for (const Case& cs : cases) {
    if (cs.vol.color_type == 1 && cs.frames.size() >= 2 && !rgb) rgb = &cs;
    if (cs.vol.color_type == 2 && cs.frames.size() >= 2 && !gray) gray = &cs;
  }
  if (!rgb || !gray) return 2;
  {
    const Case& cs = *rgb;
    teaser_hip_tsdf* h = nullptr;
    if (teaser_hip_tsdf_create(&cs.vol, 0, &h) != TEASER_HIP_OK) return 2;
    const void* pd[2] = {cs.frames[0].depth.data(), cs.frames[1].depth.data()};
    const void* pc[2] = {cs.frames[0].color.data(), cs.frames[1].color.data()};
    const void* half[2] = {cs.frames[0].depth.data(), nullptr};
    auto call = [&](int which, void (*change)(teaser_tsdf_frame_c&)) {
      teaser_tsdf_frame_c fr[2] = {cs.frames[0].f, cs.frames[1].f};
      change(fr[which]);
      return teaser_hip_tsdf_integrate_batch(h, 2, fr, pd, pc);
    };
    refused(h, call(1, [](teaser_tsdf_frame_c& x) { x.depth_format = 2; }), "depth_format", "frame 1");
    refused(h, call(0, [](teaser_tsdf_frame_c& x) { x.color_format = 4; }), "color_format", "frame 0");
    refused(h, call(1, [](teaser_tsdf_frame_c& x) { x.color_format = 2; }), "RGB8", "frame 1");
    refused(h, call(0, [](teaser_tsdf_frame_c& x) { x.color_format = 0; }), "RGB8", "frame 0");
    refused(h, call(0, [](teaser_tsdf_frame_c& x) { x.fx = 0.0; }), "fx and fy", "frame 0");
    refused(h, call(1, [](teaser_tsdf_frame_c& x) { x.fy = NAN; }), "fx and fy", "frame 1");
    refused(h, call(1, [](teaser_tsdf_frame_c& x) { x.cx = INFINITY; }), "cx and cy", "frame 1");
    refused(h, call(0, [](teaser_tsdf_frame_c& x) { x.extrinsic[7] = NAN; }), "extrinsic", "frame 0");
    refused(h, call(1, [](teaser_tsdf_frame_c& x) { x.depth_scale = 0.0; }), "depth_scale", "frame 1");
    refused(h, call(0, [](teaser_tsdf_frame_c& x) { x.depth_scale = INFINITY; }), "depth_scale", "frame 0");
    refused(h, call(1, [](teaser_tsdf_frame_c& x) { x.depth_trunc = NAN; }), "depth_trunc", "frame 1");
    refused(h, call(1, [](teaser_tsdf_frame_c& x) { x.depth_row_bytes = x.width * (x.depth_format ? 4 : 2) - 1; }), "depth_row_bytes", "frame 1");
    refused(h, call(0, [](teaser_tsdf_frame_c& x) { x.color_row_bytes = 3 * x.width - 1; }), "color_row_bytes", "frame 0");
    refused(h, call(1, [](teaser_tsdf_frame_c& x) { x.width = 16385; }), "width and height", "frame 1");
    refused(h, call(0, [](teaser_tsdf_frame_c& x) { x.height = -1; }), "width and height", "frame 0");
    teaser_tsdf_frame_c fr[2] = {cs.frames[0].f, cs.frames[1].f};
    refused(h, teaser_hip_tsdf_integrate_batch(h, 2, fr, half, pc), "depth is NULL", "frame 1");
    refused(h, teaser_hip_tsdf_integrate_batch(h, 2, fr, nullptr, pc), "depth is NULL", "frame 0");
    refused(h, teaser_hip_tsdf_integrate_batch(h, 2, fr, pd, nullptr), "color is NULL", "frame 0");
    refused(h, teaser_hip_tsdf_integrate_batch(h, 2, nullptr, pd, pc), "frames must not be NULL", "");
    refused(h, teaser_hip_tsdf_integrate_batch(h, -1, fr, pd, pc), "n_frames", "");
    expect(teaser_hip_tsdf_integrate_batch(nullptr, 2, fr, pd, pc) == TEASER_HIP_ERR_BAD_ARG, "refusal: handle", -1);
    g_integrate_launches = 0;
    expect(teaser_hip_tsdf_integrate_batch(h, 0, nullptr, nullptr, nullptr) == TEASER_HIP_OK && g_integrate_launches == 0, "no frames", -1);
    int64_t count = -5;
    std::vector<double> room(30);
    refused(h, teaser_hip_tsdf_extract_point_cloud(h, 10, nullptr, nullptr, nullptr, &count), "points must not be NULL", "");
    refused(h, teaser_hip_tsdf_extract_point_cloud(h, -1, room.data(), nullptr, nullptr, &count), "capacity", "");
    refused(h, teaser_hip_tsdf_extract_point_cloud(h, 10, room.data(), nullptr, nullptr, nullptr), "count_out", "");
    refused(h, teaser_hip_tsdf_extract_voxel_point_cloud(h, 10, nullptr, nullptr, &count), "points must not be NULL", "");
    refused(h, teaser_hip_tsdf_download(h, nullptr, nullptr), "both NULL", "");
    refused(h, teaser_hip_tsdf_upload(h, nullptr, nullptr), "both NULL", "");
    std::vector<float> bad_tw = cs.tw;
    bad_tw[3] = NAN;
    refused(h, teaser_hip_tsdf_upload(h, bad_tw.data(), nullptr), "tsdf_weight has a non-finite", "");
    std::vector<double> bad_c = cs.color;
    bad_c[4] = INFINITY;
    refused(h, teaser_hip_tsdf_upload(h, nullptr, bad_c.data()), "color has a non-finite", "");
    expect(teaser_hip_tsdf_extract_point_cloud(nullptr, 0, nullptr, nullptr, nullptr, &count) == TEASER_HIP_ERR_BAD_ARG &&
               teaser_hip_tsdf_extract_voxel_point_cloud(nullptr, 0, nullptr, nullptr, &count) == TEASER_HIP_ERR_BAD_ARG &&
               teaser_hip_tsdf_download(nullptr, nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG &&
               teaser_hip_tsdf_upload(nullptr, nullptr, nullptr) == TEASER_HIP_ERR_BAD_ARG &&
               teaser_hip_tsdf_reset(nullptr) == TEASER_HIP_ERR_BAD_ARG && teaser_hip_tsdf_destroy(nullptr) == TEASER_HIP_OK,
           "refusal: NULL handles", -1);
    // frames without pixels need no pointer and touch nothing; then the handle still works: nothing above left a trace
    teaser_tsdf_frame_c none[2] = {cs.frames[0].f, cs.frames[1].f};
    none[0].width = 0, none[1].height = 0;
    expect(teaser_hip_tsdf_integrate_batch(h, 2, none, nullptr, nullptr) == TEASER_HIP_OK, "frames without pixels", -1);
    expect(teaser_hip_tsdf_extract_voxel_point_cloud(h, 0, nullptr, nullptr, &count) == TEASER_HIP_OK && count == 0, "the refused calls touched nothing", -1);
    std::vector<teaser_tsdf_frame_c> recs;
    for (const Frame& x : cs.frames) recs.push_back(x.f);
    const std::vector<const void*> d = ptrs(cs.frames, false), c = ptrs(cs.frames, true);
    expect(teaser_hip_tsdf_integrate_batch(h, (int)recs.size(), recs.data(), d.data(), c.data()) == TEASER_HIP_OK, "the handle works afterwards", -1);
    check_volume(h, cs, -1, "after the refusals");
    teaser_hip_tsdf_destroy(h);
  }
  {
    const Case& cs = *gray;
    teaser_hip_tsdf* h = nullptr;
    if (teaser_hip_tsdf_create(&cs.vol, 0, &h) != TEASER_HIP_OK) return 2;
    const void* pd[1] = {cs.frames[0].depth.data()};
    const void* pc[1] = {cs.frames[0].color.data()};
    teaser_tsdf_frame_c fr = cs.frames[0].f;
    fr.color_format = 1;
    refused(h, teaser_hip_tsdf_integrate_batch(h, 1, &fr, pd, pc), "Gray32", "frame 0");
    teaser_hip_tsdf_destroy(h);
    // a volume without colour: the colour arguments are not read, colour outputs are refused
    teaser_tsdf_volume_c plain = cs.vol;
    plain.color_type = 0;
    if (teaser_hip_tsdf_create(&plain, 0, &h) != TEASER_HIP_OK) return 2;
    fr.color_format = 3, fr.color_row_bytes = 0;
    expect(teaser_hip_tsdf_integrate_batch(h, 1, &fr, pd, nullptr) == TEASER_HIP_OK, "a volume without colour reads no colour image", -1);
    int64_t count = 0;
    std::vector<double> room(3 * 3 * (size_t)cs.tw.size());
    refused(h, teaser_hip_tsdf_extract_point_cloud(h, 10, room.data(), nullptr, room.data(), &count), "without colour", "");
    refused(h, teaser_hip_tsdf_download(h, nullptr, room.data()), "without colour", "");
    refused(h, teaser_hip_tsdf_upload(h, nullptr, room.data()), "without colour", "");
    teaser_hip_tsdf_destroy(h);
  }
  std::printf("cases %d  mismatches %d\n", nc, g_bad);
  return g_bad ? 1 : 0;
}
