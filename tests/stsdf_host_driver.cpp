// Host-only check of the scalable TSDF volume (tests/test_stsdf_host.py): csrc/stsdf.hip -- the directory logic, the touch
// records, the passes, the slabs -- compiled by g++ against the HIP stand-in header (tests/hip_stub), built with
// -ffp-contract=off -fsanitize=address,undefined as a stand-alone program.  The launchers are serial loops over the
// functions of csrc/stsdf_device.h and csrc/tsdf_device.h -- the text the kernels compile -- walking frames, sampled
// pixels, blocks, columns and rows exactly as the kernels do.  "Device" buffers are host allocations of the size the host
// code asked for and every image ends with its last row's last sample, so a record, an offset or an output layout that
// is sized or addressed wrongly is an AddressSanitizer report.  Keys, voxels, counts, points, normals and colours are
// compared for equality with those of tests/stsdf_reference.py, read from a text file (hexadecimal floats).
//   stsdf_host_driver CASES.txt    exit code 0: every case equal and every refusal refused
// TEST INFRASTRUCTURE ONLY.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define __forceinline__ inline
#include "../teaser-plusplus_amd/csrc/stsdf.hip"

static int g_bad = 0, g_integrate_launches = 0;
static void expect(bool ok, const char* what, int c) {
  if (!ok) {
    std::fprintf(stderr, "case %d: %s\n", c, what);
    ++g_bad;
  }
}

namespace thip {

void launch_stsdf_touch(hipStream_t, const IcpFrameDesc* frames, int n_frames, int max_vis, const unsigned char* in,
                        double trunc, double ul, uint64_t* keys, uint32_t* vals, unsigned long long* oor) {
  for (int k = 0; k < n_frames; ++k) {
    const IcpFrameDesc& f = frames[k];
    if (f.n_vis > max_vis) std::abort();
    for (int t = 0; t < f.n_vis; ++t) {
      uint64_t key = kStsdfNoKey;
      uint32_t ext = 0;
      bool clipped;
      if (!stsdf_touch_pixel(f, in, t, trunc, ul, &key, &ext, &clipped)) key = kStsdfNoKey;
      keys[f.point_off + t] = key;
      vals[f.point_off + t] = ((uint32_t)k << 6) | ext;
      if (clipped) ++*oor;
    }
  }
}

size_t stsdf_unique_temp_bytes(int64_t) { return 64; }

hipError_t launch_stsdf_unique(hipStream_t, int64_t n, void*, size_t, uint64_t* keys, uint32_t* vals, uint64_t* tmp_keys,
                               uint32_t* tmp_vals, int32_t* head, int32_t* pos, uint64_t* ukeys, uint32_t* uvals,
                               int32_t* count) {
  std::vector<int64_t> order((size_t)n);
  for (int64_t k = 0; k < n; ++k) order[(size_t)k] = k, tmp_keys[k] = keys[k], tmp_vals[k] = vals[k];
  std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
    return tmp_keys[a] != tmp_keys[b] ? tmp_keys[a] < tmp_keys[b] : (tmp_vals[a] != tmp_vals[b] ? tmp_vals[a] < tmp_vals[b] : a < b);
  });
  int32_t run = 0;
  for (int64_t k = 0; k < n; ++k) {
    keys[k] = tmp_keys[order[(size_t)k]], vals[k] = tmp_vals[order[(size_t)k]];
    head[k] = keys[k] != kStsdfNoKey && (k == 0 || keys[k - 1] != keys[k] || vals[k - 1] != vals[k]) ? 1 : 0;
    run += head[k];
    pos[k] = run;
    if (head[k]) ukeys[run - 1] = keys[k], uvals[run - 1] = vals[k];
  }
  *count = run;
  return hipSuccess;
}

void launch_stsdf_integrate(hipStream_t, const TsdfGrid& g0, double ul, const TsdfChunkArgs& ck, const unsigned char* in,
                            const StsdfItem* items, int n_items) {
  ++g_integrate_launches;
  if (ck.n < 1 || ck.n > kTsdfChunk || n_items < 1) std::abort();
  for (int e = 0; e < n_items; ++e) {
    const StsdfItem& item = items[e];
    if (item.mask == 0 || (item.mask >> ck.n) != 0) std::abort();  // an item is touched, and only by frames of the pass
    int b[3];
    stsdf_unkey(item.key, b);
    const TsdfGrid g = stsdf_block_grid(g0, ul, b);
    const TsdfFields v = stsdf_fields(item.base, g.color_type);
    for (int col = 0; col < kStsdfCols; ++col) {
      const int x = col / kStsdfU, y = col % kStsdfU;
      float c[kTsdfChunk][3];
      for (int k = 0; k < kTsdfChunk; ++k)
        if ((item.mask >> k) & 1u) tsdf_column_start(g, ck.f[k], x, y, c[k]);
      for (int z = 0; z < kStsdfU; ++z) {
        const int64_t at = (int64_t)z * kStsdfCols + col;
        if (at != tsdf_index(kStsdfU, x, y, z)) std::abort();
        bool loaded = false;
        float tv = 0.0f, wv = 0.0f;
        double cv[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < kTsdfChunk; ++k)
          if ((item.mask >> k) & 1u) {
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
}

void launch_stsdf_count(hipStream_t, const TsdfGrid& g0, const StsdfDir& d, int mode, int32_t* counts, int32_t* totals,
                        int64_t* offsets) {
  int64_t run = 0;
  for (int e = 0; e < d.n; ++e) {
    char* up[3];
    stsdf_up_blocks(d, e, up);
    const TsdfFields v = stsdf_fields(d.base[e], g0.color_type);
    int32_t total = 0;
    for (int col = 0; col < kStsdfCols; ++col) {
      int32_t rows = 0;
      for (int z = 0; z < kStsdfU; ++z) rows += stsdf_voxel_rows(g0, v, up, mode, col / kStsdfU, col % kStsdfU, z);
      counts[(int64_t)e * kStsdfCols + col] = rows;
      total += rows;
    }
    totals[e] = total;
    offsets[e] = run;
    run += total;
  }
  offsets[d.n] = run;
}

void launch_stsdf_write(hipStream_t, const TsdfGrid& g0, double ul, const StsdfDir& d, int mode, const int32_t* counts,
                        const int64_t* offsets, int64_t capacity, double* points, double* normals, double* colors) {
  if (offsets[d.n] > capacity) return;
  for (int e = 0; e < d.n; ++e) {
    char* up[3];
    stsdf_up_blocks(d, e, up);
    int64_t row = offsets[e];
    for (int col = 0; col < kStsdfCols; ++col) {
      const int64_t end = stsdf_write_column(g0, ul, d, e, up, mode, col / kStsdfU, col % kStsdfU, row, points, normals, colors);
      if (end - row != counts[(int64_t)e * kStsdfCols + col]) std::abort();  // the write pass and the count pass disagree
      row = end;
    }
    if (row != offsets[e + 1]) std::abort();
  }
}

void launch_stsdf_export(hipStream_t, int color_type, char* const* base, int n, float* tw, double* color) {
  for (int e = 0; e < n; ++e) {
    const TsdfFields v = stsdf_fields(base[e], color_type);
    for (int col = 0; col < kStsdfCols; ++col)
      for (int z = 0; z < kStsdfU; ++z) {
        const int64_t at = (int64_t)z * kStsdfCols + col, o = (int64_t)e * kStsdfVoxels + col * kStsdfU + z;
        if (tw) tw[2 * o] = v.tsdf[at], tw[2 * o + 1] = v.weight[at];
        if (color)
          for (int k = 0; k < 3; ++k) color[3 * o + k] = v.color[k * v.n + at];
      }
  }
}

void launch_stsdf_import(hipStream_t, int color_type, char* const* base, int n, const float* tw, const double* color) {
  for (int e = 0; e < n; ++e) {
    const TsdfFields v = stsdf_fields(base[e], color_type);
    for (int col = 0; col < kStsdfCols; ++col)
      for (int z = 0; z < kStsdfU; ++z) {
        const int64_t at = (int64_t)z * kStsdfCols + col, o = (int64_t)e * kStsdfVoxels + col * kStsdfU + z;
        if (tw) v.tsdf[at] = tw[2 * o], v.weight[at] = tw[2 * o + 1];
        if (color)
          for (int k = 0; k < 3; ++k) v.color[k * v.n + at] = rgbd_canonical(color[3 * o + k]);
      }
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
  teaser_stsdf_volume_c vol;
  std::vector<Frame> frames;
  std::vector<int32_t> keys;
  std::vector<float> tw;
  std::vector<double> color, pts, nrm, col, vpts, vcol;
  int64_t blocks = 0, count = 0, vcount = 0, touched = 0, opened = 0, oor = 0;
};

static void refused(teaser_hip_stsdf* h, int32_t rc, int32_t want, const char* w1, const char* w2) {
  const std::string msg = teaser_hip_stsdf_last_error(h);
  expect(rc == want && msg.find(w1) != std::string::npos && msg.find(w2) != std::string::npos,
         (std::string("refusal: ") + w1 + " / " + msg).c_str(), -1);
}

static void refused_create(void (*change)(teaser_stsdf_volume_c&), const char* word) {
  teaser_stsdf_volume_c v;
  teaser_hip_stsdf_volume_default(&v);
  change(v);
  teaser_hip_stsdf* h = (teaser_hip_stsdf*)16;
  const int32_t rc = teaser_hip_stsdf_create(&v, 0, &h);
  refused(nullptr, rc, TEASER_HIP_ERR_BAD_ARG, word, "");
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
static void check_volume(teaser_hip_stsdf* h, const Case& cs, int c, const char* when) {
  const bool colored = cs.vol.color_type != 0;
  const std::string tag = std::string(" (") + when + ")";
  int64_t nb = -5;
  expect(teaser_hip_stsdf_block_count(h, &nb) == TEASER_HIP_OK && nb == cs.blocks, ("block count" + tag).c_str(), c);
  if (nb != cs.blocks) return;
  const size_t n = (size_t)nb * thip::kStsdfVoxels;
  std::vector<int32_t> keys(3 * (size_t)nb, -9);
  expect(teaser_hip_stsdf_block_keys(h, nb, nb ? keys.data() : nullptr, &nb) == TEASER_HIP_OK && same(keys, cs.keys), ("keys" + tag).c_str(), c);
  std::vector<float> tw(2 * n, -7.5f);
  std::vector<double> color(colored ? 3 * n : 0, -7.5);
  if (nb > 0) {
    expect(teaser_hip_stsdf_download_blocks(h, nb, tw.data(), colored ? color.data() : nullptr, &nb) == TEASER_HIP_OK, "download", c);
    expect(same(tw, cs.tw), ("tsdf and weight bits" + tag).c_str(), c);
    if (colored) expect(same(color, cs.color), ("colour bits" + tag).c_str(), c);
  }
  int64_t count = -5;
  expect(teaser_hip_stsdf_extract_point_cloud(h, 0, nullptr, nullptr, nullptr, &count) == TEASER_HIP_OK && count == cs.count,
         ("count" + tag).c_str(), c);
  if (count != cs.count) return;
  const size_t m = (size_t)count;
  std::vector<double> p(3 * m + 3, -7.5), nn(3 * m + 3, -7.5), cc(3 * m + 3, -7.5);
  count = -5;
  expect(teaser_hip_stsdf_extract_point_cloud(h, (int64_t)m, p.data(), nn.data(), colored ? cc.data() : nullptr, &count) == TEASER_HIP_OK &&
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
    refused(h, teaser_hip_stsdf_extract_point_cloud(h, (int64_t)m - 1, q.data(), qn.data(), nullptr, &count), TEASER_HIP_ERR_BAD_ARG,
            "capacity", ("count " + std::to_string(m)).c_str());
    expect(count == cs.count, "the refused extraction reports the count", c);
    expect(q == std::vector<double>(3 * m, -7.5) && qn == q, "the refused extraction writes nothing", c);
  }
  int64_t vcount = -5;
  expect(teaser_hip_stsdf_extract_voxel_point_cloud(h, 0, nullptr, nullptr, &vcount) == TEASER_HIP_OK && vcount == cs.vcount,
         ("voxel count" + tag).c_str(), c);
  if (vcount != cs.vcount) return;
  std::vector<double> vp(3 * (size_t)vcount, -7.5), vc(3 * (size_t)vcount, -7.5);
  expect(teaser_hip_stsdf_extract_voxel_point_cloud(h, vcount, vcount ? vp.data() : nullptr, vcount ? vc.data() : nullptr, &vcount) ==
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
    if (teaser_hip_stsdf_volume_default(&cs.vol) != TEASER_HIP_OK) return 2;
    cs.vol.color_type = (int)read_number(f), cs.vol.depth_sampling_stride = (int)read_number(f);
    cs.frames.resize((size_t)read_number(f));
    cs.vol.voxel_length = read_number(f), cs.vol.sdf_trunc = read_number(f);
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
    cs.blocks = (int64_t)read_number(f);
    const size_t n = (size_t)cs.blocks * thip::kStsdfVoxels;
    read_numbers(f, cs.keys, 3 * (size_t)cs.blocks);
    read_numbers(f, cs.tw, 2 * n);
    if (cs.vol.color_type) read_numbers(f, cs.color, 3 * n);
    cs.count = (int64_t)read_number(f);
    read_numbers(f, cs.pts, 3 * (size_t)cs.count);
    read_numbers(f, cs.nrm, 3 * (size_t)cs.count);
    if (cs.vol.color_type) read_numbers(f, cs.col, 3 * (size_t)cs.count);
    cs.vcount = (int64_t)read_number(f);
    read_numbers(f, cs.vpts, 3 * (size_t)cs.vcount);
    read_numbers(f, cs.vcol, 3 * (size_t)cs.vcount);
    cs.touched = (int64_t)read_number(f), cs.opened = (int64_t)read_number(f), cs.oor = (int64_t)read_number(f);
  }
  std::fclose(f);

  for (int c = 0; c < nc; ++c) {
    const Case& cs = cases[(size_t)c];
    const int nf = (int)cs.frames.size();
    teaser_stsdf_volume_c tight = cs.vol;  // b grows a block at a time
    tight.initial_blocks = 1, tight.slab_blocks = 1;
    teaser_hip_stsdf *a = nullptr, *b = nullptr;  // two volumes alive at once
    if (teaser_hip_stsdf_create(&cs.vol, 0, &a) != TEASER_HIP_OK || teaser_hip_stsdf_create(&tight, -1, &b) != TEASER_HIP_OK) return 2;
    std::vector<teaser_tsdf_frame_c> recs;
    for (const Frame& fr : cs.frames) recs.push_back(fr.f);
    const std::vector<const void*> pd = ptrs(cs.frames, false), pc = ptrs(cs.frames, true);
    // a: every frame in one call; b: one call per frame
    int64_t touched = -1, opened = -1, oor = -1;
    g_integrate_launches = 0;
    expect(teaser_hip_stsdf_integrate_frames(a, nf, recs.data(), pd.data(), pc.data(), &touched, &opened, &oor) == TEASER_HIP_OK,
           teaser_hip_stsdf_last_error(a), c);
    expect(touched == cs.touched && opened == cs.opened && oor == cs.oor, "touched, opened and out_of_range of one call", c);
    expect(g_integrate_launches <= (nf + thip::kTsdfChunk - 1) / thip::kTsdfChunk, "at most one launch per pass of frames", c);
    int64_t sums[3] = {0, 0, 0};
    for (int k = 0; k < nf; ++k) {
      expect(teaser_hip_stsdf_integrate_frames(b, 1, &recs[(size_t)k], &pd[(size_t)k], &pc[(size_t)k], &touched, &opened, &oor) == TEASER_HIP_OK,
             teaser_hip_stsdf_last_error(b), c);
      sums[0] += touched, sums[1] += opened, sums[2] += oor;
    }
    expect(sums[0] == cs.touched && sums[1] == cs.opened && sums[2] == cs.oor, "the counts of a call per frame", c);
    expect((int64_t)b->slabs.size() == cs.blocks, "a slab per block when slabs hold one", c);
    check_volume(a, cs, c, "one call");
    check_volume(b, cs, c, "a call per frame");
    // reset, then the state back through upload, the blocks in reverse order
    expect(teaser_hip_stsdf_reset(b) == TEASER_HIP_OK, "reset", c);
    int64_t count = -5;
    expect(teaser_hip_stsdf_block_count(b, &count) == TEASER_HIP_OK && count == 0, "reset closes every block", c);
    expect(teaser_hip_stsdf_extract_point_cloud(b, 0, nullptr, nullptr, nullptr, &count) == TEASER_HIP_OK && count == 0, "an empty volume has no rows", c);
    if (cs.blocks > 0) {
      const size_t nb = (size_t)cs.blocks, V = thip::kStsdfVoxels;
      std::vector<int32_t> keys(3 * nb);
      std::vector<float> tw(2 * V * nb);
      std::vector<double> col(cs.vol.color_type ? 3 * V * nb : 0);
      for (size_t k = 0; k < nb; ++k) {
        const size_t s = nb - 1 - k;
        memcpy(&keys[3 * k], &cs.keys[3 * s], 12);
        memcpy(&tw[2 * V * k], &cs.tw[2 * V * s], 8 * V);
        if (cs.vol.color_type) memcpy(&col[3 * V * k], &cs.color[3 * V * s], 24 * V);
      }
      expect(teaser_hip_stsdf_upload_blocks(b, (int64_t)nb, keys.data(), tw.data(), cs.vol.color_type ? col.data() : nullptr) == TEASER_HIP_OK, "upload", c);
      check_volume(b, cs, c, "after reset and upload");
      if (nb >= 2) {
        memcpy(&keys[3], &keys[0], 12);
        refused(b, teaser_hip_stsdf_upload_blocks(b, 2, keys.data(), tw.data(), nullptr), TEASER_HIP_ERR_BAD_ARG, "occurs twice", "");
      }
      keys[1] = 1 << 20;
      refused(b, teaser_hip_stsdf_upload_blocks(b, 1, keys.data(), tw.data(), nullptr), TEASER_HIP_ERR_BAD_ARG, "outside", "block 0");
      // max_blocks one below what the case needs: OOM, nothing changed, and a smaller call succeeds
      teaser_stsdf_volume_c capped = cs.vol;
      capped.max_blocks = cs.blocks - 1;
      teaser_hip_stsdf* m = nullptr;
      if (capped.max_blocks > 0 && nf > 1) {
        if (teaser_hip_stsdf_create(&capped, 0, &m) != TEASER_HIP_OK) return 2;
        int k = 0;
        int32_t rc = TEASER_HIP_OK;
        for (; k < nf && rc == TEASER_HIP_OK; ++k)
          rc = teaser_hip_stsdf_integrate_frames(m, 1, &recs[(size_t)k], &pd[(size_t)k], &pc[(size_t)k], nullptr, &opened, nullptr);
        refused(m, rc, TEASER_HIP_ERR_OOM, "max_blocks", "");
        expect(opened == 0, "a refused call opens nothing", c);
        int64_t before = -1;
        teaser_hip_stsdf_block_count(m, &before);
        expect(before < cs.blocks && teaser_hip_stsdf_integrate_frames(m, 1, &recs[0], &pd[0], &pc[0], nullptr, &opened, nullptr) == TEASER_HIP_OK &&
                   opened == 0, "the handle works after the OOM", c);
        teaser_hip_stsdf_destroy(m);
      }
    }
    teaser_hip_stsdf_destroy(a);
    teaser_hip_stsdf_destroy(b);
  }

  // refusals: BAD_ARG with the argument (and the frame) named; the handle stays usable
  refused_create([](teaser_stsdf_volume_c& v) { v.volume_unit_resolution = 8; }, "supports only 16");
  refused_create([](teaser_stsdf_volume_c& v) { v.volume_unit_resolution = 12; }, "power of two");
  refused_create([](teaser_stsdf_volume_c& v) { v.voxel_length = 0.0; }, "voxel_length");
  refused_create([](teaser_stsdf_volume_c& v) { v.voxel_length = INFINITY; }, "voxel_length");
  refused_create([](teaser_stsdf_volume_c& v) { v.sdf_trunc = -0.1; }, "sdf_trunc");
  refused_create([](teaser_stsdf_volume_c& v) { v.sdf_trunc = NAN; }, "sdf_trunc");
  refused_create([](teaser_stsdf_volume_c& v) { v.sdf_trunc = v.voxel_length * 16.5; }, "block's side");
  refused_create([](teaser_stsdf_volume_c& v) { v.color_type = 3; }, "color_type");
  refused_create([](teaser_stsdf_volume_c& v) { v.depth_sampling_stride = 0; }, "depth_sampling_stride");
  refused_create([](teaser_stsdf_volume_c& v) { v.initial_blocks = 0; }, "initial_blocks");
  refused_create([](teaser_stsdf_volume_c& v) { v.slab_blocks = -1; }, "slab_blocks");
  refused_create([](teaser_stsdf_volume_c& v) { v.max_blocks = -1; }, "max_blocks");
  refused_create([](teaser_stsdf_volume_c& v) { v.reserved = 1; }, "reserved");
  refused_create([](teaser_stsdf_volume_c& v) { v.reserved32 = 1; }, "reserved");
  {
    teaser_stsdf_volume_c v;
    teaser_hip_stsdf_volume_default(&v);
    v.sdf_trunc = v.voxel_length * 16.0;  // exactly a block's side is legal
    teaser_hip_stsdf* h = nullptr;
    expect(teaser_hip_stsdf_create(&v, 0, &h) == TEASER_HIP_OK && h, "sdf_trunc = ul", -1);
    teaser_hip_stsdf_destroy(h);
  }
  const Case* rgb = nullptr;
  for (const Case& cs : cases)
    if (cs.vol.color_type == 1 && cs.frames.size() >= 2 && cs.blocks > 0 && !rgb) rgb = &cs;
  if (!rgb) return 2;
  {
    const Case& cs = *rgb;
    teaser_hip_stsdf* h = nullptr;
    if (teaser_hip_stsdf_create(&cs.vol, 0, &h) != TEASER_HIP_OK) return 2;
    const void* pd[2] = {cs.frames[0].depth.data(), cs.frames[1].depth.data()};
    const void* pc[2] = {cs.frames[0].color.data(), cs.frames[1].color.data()};
    auto call = [&](int which, void (*change)(teaser_tsdf_frame_c&)) {
      teaser_tsdf_frame_c fr[2] = {cs.frames[0].f, cs.frames[1].f};
      change(fr[which]);
      return teaser_hip_stsdf_integrate_frames(h, 2, fr, pd, pc, nullptr, nullptr, nullptr);
    };
    const int32_t B = TEASER_HIP_ERR_BAD_ARG;
    refused(h, call(1, [](teaser_tsdf_frame_c& x) { x.depth_format = 2; }), B, "depth_format", "frame 1");
    refused(h, call(0, [](teaser_tsdf_frame_c& x) { x.color_format = 2; }), B, "RGB8", "frame 0");
    refused(h, call(0, [](teaser_tsdf_frame_c& x) { x.fx = 0.0; }), B, "fx and fy", "frame 0");
    refused(h, call(1, [](teaser_tsdf_frame_c& x) { x.extrinsic[7] = NAN; }), B, "extrinsic", "frame 1");
    refused(h, call(1, [](teaser_tsdf_frame_c& x) { for (int k = 0; k < 3; ++k) x.extrinsic[8 + k] = 0.0; }), B, "singular", "frame 1");
    refused(h, call(0, [](teaser_tsdf_frame_c& x) { x.depth_scale = 0.0; }), B, "depth_scale", "frame 0");
    refused(h, call(1, [](teaser_tsdf_frame_c& x) { x.depth_row_bytes = x.width * (x.depth_format ? 4 : 2) - 1; }), B, "depth_row_bytes", "frame 1");
    refused(h, call(0, [](teaser_tsdf_frame_c& x) { x.height = -1; }), B, "width and height", "frame 0");
    teaser_tsdf_frame_c fr[2] = {cs.frames[0].f, cs.frames[1].f};
    refused(h, teaser_hip_stsdf_integrate_frames(h, 2, fr, nullptr, pc, nullptr, nullptr, nullptr), B, "depth is NULL", "frame 0");
    refused(h, teaser_hip_stsdf_integrate_frames(h, 2, fr, pd, nullptr, nullptr, nullptr, nullptr), B, "color is NULL", "frame 0");
    refused(h, teaser_hip_stsdf_integrate_frames(h, 2, nullptr, pd, pc, nullptr, nullptr, nullptr), B, "frames must not be NULL", "");
    refused(h, teaser_hip_stsdf_integrate_frames(h, -1, fr, pd, pc, nullptr, nullptr, nullptr), B, "n_frames", "");
    refused(h, teaser_hip_stsdf_integrate_frames(h, 65536, fr, pd, pc, nullptr, nullptr, nullptr), TEASER_HIP_ERR_UNSUPPORTED, "65535", "");
    g_integrate_launches = 0;
    expect(teaser_hip_stsdf_integrate_frames(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == TEASER_HIP_OK && g_integrate_launches == 0, "no frames", -1);
    int64_t count = -5;
    std::vector<double> room(30);
    refused(h, teaser_hip_stsdf_extract_point_cloud(h, 10, nullptr, nullptr, nullptr, &count), B, "points must not be NULL", "");
    refused(h, teaser_hip_stsdf_extract_point_cloud(h, -1, room.data(), nullptr, nullptr, &count), B, "capacity", "");
    refused(h, teaser_hip_stsdf_extract_point_cloud(h, 10, room.data(), nullptr, nullptr, nullptr), B, "count_out", "");
    refused(h, teaser_hip_stsdf_block_keys(h, 3, nullptr, &count), B, "keys must not be NULL", "");
    refused(h, teaser_hip_stsdf_block_count(h, nullptr), B, "count_out", "");
    refused(h, teaser_hip_stsdf_upload_blocks(h, 1, nullptr, cs.tw.data(), nullptr), B, "keys must not be NULL", "");
    refused(h, teaser_hip_stsdf_upload_blocks(h, 1, cs.keys.data(), nullptr, nullptr), B, "both NULL", "");
    std::vector<float> bad_tw(cs.tw.begin(), cs.tw.begin() + 2 * thip::kStsdfVoxels);
    bad_tw[3] = NAN;
    refused(h, teaser_hip_stsdf_upload_blocks(h, 1, cs.keys.data(), bad_tw.data(), nullptr), B, "tsdf_weight has a non-finite", "");
    expect(teaser_hip_stsdf_block_count(h, &count) == TEASER_HIP_OK && count == 0, "the refused calls opened nothing", -1);
    expect(teaser_hip_stsdf_extract_point_cloud(nullptr, 0, nullptr, nullptr, nullptr, &count) == B &&
               teaser_hip_stsdf_reset(nullptr) == B && teaser_hip_stsdf_destroy(nullptr) == TEASER_HIP_OK &&
               teaser_hip_stsdf_integrate_frames(nullptr, 2, fr, pd, pc, nullptr, nullptr, nullptr) == B, "refusal: NULL handles", -1);
    // frames without pixels need no pointer and touch nothing; then the handle still works
    teaser_tsdf_frame_c none[2] = {cs.frames[0].f, cs.frames[1].f};
    none[0].width = 0, none[1].height = 0;
    int64_t touched = -1;
    expect(teaser_hip_stsdf_integrate_frames(h, 2, none, nullptr, nullptr, &touched, nullptr, nullptr) == TEASER_HIP_OK && touched == 0, "frames without pixels", -1);
    std::vector<teaser_tsdf_frame_c> recs;
    for (const Frame& x : cs.frames) recs.push_back(x.f);
    const std::vector<const void*> d = ptrs(cs.frames, false), cc = ptrs(cs.frames, true);
    expect(teaser_hip_stsdf_integrate_frames(h, (int)recs.size(), recs.data(), d.data(), cc.data(), nullptr, nullptr, nullptr) == TEASER_HIP_OK, "the handle works afterwards", -1);
    check_volume(h, cs, -1, "after the refusals");
    teaser_hip_stsdf_destroy(h);
  }
  std::printf("cases %d  mismatches %d\n", nc, g_bad);
  return g_bad ? 1 : 0;
}
