// stsdf.hip -- host side of the scalable TSDF volume (include/teaser_hip.h, "Scalable TSDF volume"): the handle, the
// directory of open blocks -- which the host owns -- and the entry checks.  Kernels: kernels_stsdf.hip; device code:
// stsdf_device.h; design, bytes moved and the resource report: DESIGN.md section 37.
//
// Integration: the images go up as in the dense volume (tsdf_internal.h), with one touch record per frame behind them.
// The touch pass leaves one candidate per sampled pixel, the unique pass the distinct ones; those come back (the first
// synchronisation).  The host expands every candidate's box of blocks, merges the new blocks into the directory -- slots
// in ascending key order, slabs allocated as needed, everything that can fail before anything changes -- zeroes the new
// blocks and lists, per pass of kTsdfChunk frames, the blocks that pass touches with their frame masks.  One launch per
// pass, and the second synchronisation.  Extraction: count, scan and write over the directory, as the dense volume does
// over its columns.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <unordered_map>
#include <vector>

#include "stsdf_internal.h"

using namespace thip;

namespace {

thread_local std::string g_stsdf_create_error;  // what teaser_hip_stsdf_last_error(NULL) returns

constexpr int64_t kReadback = 262144;  // distinct candidates the first copy brings back; more cost a second copy
constexpr int kBatchBlocks = 256;     // blocks one step of download and upload moves

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int32_t refuse_stsdf_create(const std::string& msg) {
  g_stsdf_create_error = msg;
  return TEASER_HIP_ERR_BAD_ARG;
}

// camera_pose = the inverse of the extrinsic by the closed form of the contract; false: singular.
bool invert_extrinsic(const double* E, double* M) {
  const double A00 = E[0], A01 = E[1], A02 = E[2], A10 = E[4], A11 = E[5], A12 = E[6], A20 = E[8], A21 = E[9], A22 = E[10];
  const double t[3] = {E[3], E[7], E[11]};
  const double c[3][3] = {{A11 * A22 - A12 * A21, A12 * A20 - A10 * A22, A10 * A21 - A11 * A20},
                          {A02 * A21 - A01 * A22, A00 * A22 - A02 * A20, A01 * A20 - A00 * A21},
                          {A01 * A12 - A02 * A11, A02 * A10 - A00 * A12, A00 * A11 - A01 * A10}};
  const double det = (A00 * c[0][0] + A01 * c[0][1]) + A02 * c[0][2];
  if (det == 0.0 || !std::isfinite(det)) return false;
  for (int r = 0; r < 3; ++r) {
    double* m = M + 4 * r;
    for (int k = 0; k < 3; ++k) m[k] = c[k][r] / det;
    m[3] = -((m[0] * t[0] + m[1] * t[1]) + m[2] * t[2]);
    for (int k = 0; k < 4; ++k)
      if (!std::isfinite(m[k])) return false;
  }
  return true;
}

// Opens the blocks `fresh` (ascending, none of them open): everything that can fail comes first, so a refusal leaves
// the directory and every voxel as they were.  The new blocks take the next slots in key order and are zeroed.
int32_t open_blocks(teaser_hip_stsdf* h, const std::vector<uint64_t>& fresh) {
  if (fresh.empty()) return TEASER_HIP_OK;
  const int64_t old_n = (int64_t)h->keys.size(), new_n = old_n + (int64_t)fresh.size();
  if (h->vol.max_blocks > 0 && new_n > h->vol.max_blocks)
    return fail(h, TEASER_HIP_ERR_OOM, "the call would open block " + std::to_string(new_n) + " of at most max_blocks = " +
                                           std::to_string(h->vol.max_blocks));
  if (new_n > INT32_MAX) return fail(h, TEASER_HIP_ERR_OOM, "more than 2^31 - 1 blocks");
  while (stsdf_capacity(h) < new_n) {  // a slab allocated here stays, used or not
    const size_t bytes = (size_t)(h->slabs.empty() ? h->vol.initial_blocks : h->vol.slab_blocks) * h->block_bytes;
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (a slab of " + std::to_string(bytes) + " bytes)");
    }
    h->slabs.push_back(p);
  }
  std::vector<uint64_t> keys((size_t)new_n);
  std::vector<int32_t> slots((size_t)new_n);
  size_t a = 0, b = 0, o = 0;
  while (a < h->keys.size() || b < fresh.size()) {
    if (b == fresh.size() || (a < h->keys.size() && h->keys[a] < fresh[b])) {
      keys[o] = h->keys[a], slots[o] = h->slots[a], ++a;
    } else {
      keys[o] = fresh[b], slots[o] = (int32_t)(old_n + (int64_t)b), ++b;
    }
    ++o;
  }
  h->keys.swap(keys);
  h->slots.swap(slots);
  h->dir_dirty = true;
  for (int64_t slot = old_n; slot < new_n;) {  // the new slots are consecutive: one fill per slab they reach into
    const int64_t first = h->vol.initial_blocks;
    const int64_t slab_end = slot < first ? first : first + ((slot - first) / h->vol.slab_blocks + 1) * h->vol.slab_blocks;
    const int64_t end = std::min(new_n, slab_end);
    FCHK(h, hipMemsetAsync(stsdf_block_ptr(h, slot), 0, (size_t)(end - slot) * h->block_bytes, h->stream),
         "hipMemsetAsync (new blocks)");
    slot = end;
  }
  return TEASER_HIP_OK;
}

}  // namespace

// The device copy of the directory: keys, then the blocks' addresses, both in key order; uploaded only when the
// directory has changed since the last upload.  stsdf_raycast.hip calls it, too.
int32_t thip::stsdf_sync_directory(teaser_hip_stsdf* h, StsdfDir* d) {
  const size_t n = h->keys.size();
  const size_t o_base = round_up(sizeof(uint64_t) * std::max<size_t>(n, 1), 256);
  if (h->dir_dirty) {
    const size_t bytes = o_base + sizeof(char*) * std::max<size_t>(n, 1);
    if (!h->dir.ensure(bytes) || !h->istage.ensure(bytes))
      return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (block directory)");
    char* st = h->istage.as<char>();
    if (n > 0) memcpy(st, h->keys.data(), sizeof(uint64_t) * n);
    char** base = reinterpret_cast<char**>(st + o_base);
    for (size_t k = 0; k < n; ++k) base[k] = stsdf_block_ptr(h, h->slots[k]);
    FCHK(h, hipMemcpyAsync(h->dir.p, st, bytes, hipMemcpyHostToDevice, h->stream), "hipMemcpyAsync (block directory)");
    h->dir_dirty = false;
  }
  d->keys = h->dir.as<uint64_t>();
  d->base = reinterpret_cast<char* const*>(h->dir.as<char>() + o_base);
  d->n = (int32_t)n;
  return TEASER_HIP_OK;
}

namespace {

int32_t integrate(teaser_hip_stsdf* h, int32_t n_frames, const teaser_tsdf_frame_c* frames, const void* const* depth,
                  const void* const* color, int64_t* touched_out, int64_t* opened_out, int64_t* oor_out) {
  if (touched_out) *touched_out = 0;
  if (opened_out) *opened_out = 0;
  if (oor_out) *oor_out = 0;
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (n_frames < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_frames must be >= 0");
  if (n_frames == 0) return TEASER_HIP_OK;
  if (!frames) return fail(h, TEASER_HIP_ERR_BAD_ARG, "frames must not be NULL");
  if (n_frames > kStsdfMaxFrames)
    return fail(h, TEASER_HIP_ERR_UNSUPPORTED, "a call takes at most 65535 frames; split longer sequences across calls");
  const TsdfGrid& g = h->g;
  const auto t_start = std::chrono::steady_clock::now();
  h->phase_ms[0] = h->phase_ms[1] = h->phase_ms[2] = 0.0;
  std::vector<TsdfFrame> fd;
  size_t in_bytes = 0;
  const int32_t rc = plan_frames(h, g, n_frames, frames, depth, color, fd, &in_bytes);
  if (rc != TEASER_HIP_OK) return rc;
  // the touch records
  const int stride = h->vol.depth_sampling_stride;
  std::vector<IcpFrameDesc> td((size_t)n_frames);
  int64_t N = 0;
  int max_vis = 0;
  for (int b = 0; b < n_frames; ++b) {
    const teaser_tsdf_frame_c& f = frames[b];
    IcpFrameDesc& d = td[(size_t)b];
    memset(&d, 0, sizeof(d));
    if (!invert_extrinsic(f.extrinsic, d.pose)) return fail(h, TEASER_HIP_ERR_BAD_ARG, "extrinsic is singular" + frame_at(b));
    d.width = f.width, d.height = f.height, d.stride = stride, d.depth_format = f.depth_format, d.valid_only = 1;
    d.nj = (f.width + stride - 1) / stride;
    d.n_vis = f.width == 0 || f.height == 0 ? 0 : ((f.height + stride - 1) / stride) * d.nj;
    d.depth_off = fd[(size_t)b].depth_off;
    d.point_off = N;
    d.color_out = d.pixel_out = -1;
    d.fx = f.fx, d.fy = f.fy, d.cx = f.cx, d.cy = f.cy;
    d.depth_trunc = f.depth_trunc, d.depth_scale = (float)f.depth_scale;
    N += d.n_vis;
    max_vis = std::max(max_vis, d.n_vis);
  }
  if (N > INT32_MAX) return fail(h, TEASER_HIP_ERR_BAD_ARG, "more than 2^31 - 1 sampled pixels in one call");
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  const size_t o_td = round_up(in_bytes, 16), all_in = o_td + sizeof(IcpFrameDesc) * (size_t)n_frames;
  if (!h->in.ensure(all_in) || !h->stage.ensure(all_in))
    return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (TSDF frame buffers)");
  unsigned char* stage = h->stage.as<unsigned char>();
  stage_frames(g, n_frames, frames, depth, color, fd, stage);
  memcpy(stage + o_td, td.data(), sizeof(IcpFrameDesc) * (size_t)n_frames);
  hipStream_t s = h->stream;
  FCHK(h, hipMemcpyAsync(h->in.p, stage, all_in, hipMemcpyHostToDevice, s), "hipMemcpyAsync (frames)");
  const unsigned char* d_in = h->in.as<unsigned char>();

  // touch, unique, and the distinct candidates back
  const size_t n = (size_t)N, o_hdr = 256;
  int32_t n_cand = 0;
  unsigned long long oor = 0;
  const uint64_t* ukeys = nullptr;
  const uint32_t* uvals = nullptr;
  if (N > 0) {
    const size_t o_skeys = 8 * n, o_vals = 16 * n, o_svals = 20 * n, o_head = 24 * n, o_pos = 28 * n;
    const size_t o_temp = round_up(32 * n, 256), temp_bytes = stsdf_unique_temp_bytes(N);
    const size_t o_uvals = o_hdr + 8 * n;
    if (!h->work.ensure(o_temp + std::max<size_t>(temp_bytes, 16)) || !h->out.ensure(o_uvals + 4 * n))
      return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (touch buffers)");
    char* w = h->work.as<char>();
    char* out = h->out.as<char>();
    int32_t* d_count = reinterpret_cast<int32_t*>(out);
    unsigned long long* d_oor = reinterpret_cast<unsigned long long*>(out + 8);
    FCHK(h, hipMemsetAsync(out, 0, 16, s), "hipMemsetAsync (touch counters)");
    launch_stsdf_touch(s, reinterpret_cast<const IcpFrameDesc*>(d_in + o_td), n_frames, max_vis, d_in, h->vol.sdf_trunc,
                       h->ul, reinterpret_cast<uint64_t*>(w), reinterpret_cast<uint32_t*>(w + o_vals), d_oor);
    FCHK(h, launch_stsdf_unique(s, N, w + o_temp, temp_bytes, reinterpret_cast<uint64_t*>(w),
                                reinterpret_cast<uint32_t*>(w + o_vals), reinterpret_cast<uint64_t*>(w + o_skeys),
                                reinterpret_cast<uint32_t*>(w + o_svals), reinterpret_cast<int32_t*>(w + o_head),
                                reinterpret_cast<int32_t*>(w + o_pos), reinterpret_cast<uint64_t*>(out + o_hdr),
                                reinterpret_cast<uint32_t*>(out + o_uvals), d_count),
         "the unique pass");
    FCHK(h, hipGetLastError(), "kernel launch (touch pass)");
    const size_t m0 = (size_t)std::min<int64_t>(N, kReadback);
    if (!h->back.ensure(o_hdr + 12 * m0)) return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (touch read-back)");
    char* back = h->back.as<char>();
    FCHK(h, hipMemcpyAsync(back, out, 16, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (touch counters)");
    FCHK(h, hipMemcpyAsync(back + o_hdr, out + o_hdr, 8 * m0, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (candidates)");
    FCHK(h, hipMemcpyAsync(back + o_hdr + 8 * m0, out + o_uvals, 4 * m0, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (candidates)");
    FCHK(h, hipStreamSynchronize(s), "touch pass");
    memcpy(&n_cand, back, sizeof(n_cand));
    memcpy(&oor, back + 8, sizeof(oor));
    size_t m = m0;
    if ((size_t)n_cand > m0) {  // rare: more distinct candidates than the first copy brought
      m = (size_t)n_cand;
      if (!h->back.ensure(o_hdr + 12 * m)) return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (touch read-back)");
      back = h->back.as<char>();
      FCHK(h, hipMemcpyAsync(back + o_hdr, out + o_hdr, 8 * m, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (candidates)");
      FCHK(h, hipMemcpyAsync(back + o_hdr + 8 * m, out + o_uvals, 4 * m, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (candidates)");
      FCHK(h, hipStreamSynchronize(s), "touch pass (second copy)");
    }
    ukeys = reinterpret_cast<const uint64_t*>(back + o_hdr);
    uvals = reinterpret_cast<const uint32_t*>(back + o_hdr + 8 * m);
  }

  h->phase_ms[0] = ms_since(t_start);
  const auto t_dir = std::chrono::steady_clock::now();
  // the boxes of the candidates: per touched block one mask byte per pass
  const int n_pass = (n_frames + kTsdfChunk - 1) / kTsdfChunk;
  std::unordered_map<uint64_t, int32_t> index;
  std::vector<uint64_t> tkeys;
  std::vector<uint8_t> masks;
  for (int32_t u = 0; u < n_cand; ++u) {
    int lo[3];
    stsdf_unkey(ukeys[u], lo);
    const uint32_t ext = uvals[u] & 63u, frame = uvals[u] >> 6;
    const int ex = (int)(ext & 3u), ey = (int)((ext >> 2) & 3u), ez = (int)((ext >> 4) & 3u);
    for (int dx = 0; dx <= ex; ++dx)
      for (int dy = 0; dy <= ey; ++dy)
        for (int dz = 0; dz <= ez; ++dz) {
          const uint64_t key = stsdf_key(lo[0] + dx, lo[1] + dy, lo[2] + dz);
          auto it = index.find(key);
          if (it == index.end()) {
            it = index.emplace(key, (int32_t)tkeys.size()).first;
            tkeys.push_back(key);
            masks.resize(masks.size() + (size_t)n_pass, 0);
          }
          masks[(size_t)it->second * (size_t)n_pass + frame / kTsdfChunk] |= (uint8_t)(1u << (frame % kTsdfChunk));
        }
  }
  std::vector<int32_t> order(tkeys.size());
  for (size_t k = 0; k < order.size(); ++k) order[k] = (int32_t)k;
  std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return tkeys[(size_t)a] < tkeys[(size_t)b]; });
  std::vector<uint64_t> fresh;
  int64_t touched = 0, n_items = 0;
  for (int32_t k : order) {
    if (!std::binary_search(h->keys.begin(), h->keys.end(), tkeys[(size_t)k])) fresh.push_back(tkeys[(size_t)k]);
    for (int p = 0; p < n_pass; ++p) {
      const uint8_t mk = masks[(size_t)k * (size_t)n_pass + (size_t)p];
      touched += __builtin_popcount(mk);
      n_items += mk != 0;
    }
  }
  // everything that can fail, then the directory, then the voxels
  const size_t item_bytes = sizeof(StsdfItem) * (size_t)std::max<int64_t>(n_items, 1);
  if (!h->items.ensure(item_bytes) || !h->istage.ensure(item_bytes))
    return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (integration items)");
  const int32_t rc_open = open_blocks(h, fresh);
  if (rc_open != TEASER_HIP_OK) return rc_open;
  StsdfItem* items = h->istage.as<StsdfItem>();
  std::vector<int64_t> pass_off((size_t)n_pass + 1, 0);
  int64_t at = 0;
  for (int p = 0; p < n_pass; ++p) {
    pass_off[(size_t)p] = at;
    for (int32_t k : order) {
      const uint8_t mk = masks[(size_t)k * (size_t)n_pass + (size_t)p];
      if (!mk) continue;
      const size_t e = (size_t)(std::lower_bound(h->keys.begin(), h->keys.end(), tkeys[(size_t)k]) - h->keys.begin());
      items[at].key = tkeys[(size_t)k];
      items[at].base = stsdf_block_ptr(h, h->slots[e]);
      items[at].mask = mk;
      items[at].pad = 0;
      ++at;
    }
  }
  pass_off[(size_t)n_pass] = at;
  h->phase_ms[1] = ms_since(t_dir);
  const auto t_int = std::chrono::steady_clock::now();
  if (n_items > 0) {
    FCHK(h, hipMemcpyAsync(h->items.p, items, sizeof(StsdfItem) * (size_t)n_items, hipMemcpyHostToDevice, s),
         "hipMemcpyAsync (integration items)");
    for (int p = 0; p < n_pass; ++p) {
      const int64_t cnt = pass_off[(size_t)p + 1] - pass_off[(size_t)p];
      if (cnt == 0) continue;
      TsdfChunkArgs ck;
      memset(&ck, 0, sizeof(ck));
      ck.n = std::min(kTsdfChunk, n_frames - p * kTsdfChunk);
      ck.segments = 1;
      for (int k = 0; k < ck.n; ++k) ck.f[k] = fd[(size_t)(p * kTsdfChunk + k)];
      launch_stsdf_integrate(s, g, h->ul, ck, d_in, h->items.as<StsdfItem>() + pass_off[(size_t)p], (int)cnt);
    }
    FCHK(h, hipGetLastError(), "kernel launch (scalable TSDF integration)");
  }
  FCHK(h, hipStreamSynchronize(s), "scalable TSDF integration");
  h->phase_ms[2] = ms_since(t_int);
  if (touched_out) *touched_out = touched;
  if (opened_out) *opened_out = (int64_t)fresh.size();
  if (oor_out) *oor_out = (int64_t)oor;
  return TEASER_HIP_OK;
}

// mode 0: the surface points; mode 1: the voxel cloud.
int32_t extract(teaser_hip_stsdf* h, int mode, int64_t capacity, double* points, double* normals, double* colors,
                int64_t* count_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (!count_out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "count_out must not be NULL");
  if (capacity < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "capacity must be >= 0");
  if (capacity > 0 && !points) return fail(h, TEASER_HIP_ERR_BAD_ARG, "points must not be NULL with a capacity above 0");
  if (mode == 0 && colors && h->g.color_type == 0)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "colors is given for a volume without colour");
  const int64_t nb = (int64_t)h->keys.size();
  const int64_t cap = std::min<int64_t>(capacity, (mode == 0 ? 3 : 1) * nb * kStsdfVoxels);  // no more rows can exist
  const bool want_n = cap > 0 && normals, want_c = cap > 0 && colors;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  StsdfDir d;
  const int32_t rc = stsdf_sync_directory(h, &d);
  if (rc != TEASER_HIP_OK) return rc;
  const size_t o_totals = round_up(sizeof(int64_t) * (size_t)(nb + 1), 256);
  const size_t o_counts = o_totals + round_up(sizeof(int32_t) * (size_t)std::max<int64_t>(nb, 1), 256);
  const size_t row = sizeof(double) * 3 * (size_t)cap;
  const size_t o_pts = round_up(sizeof(int64_t), 256);
  const size_t o_norm = o_pts + row, o_col = o_norm + (want_n ? row : 0), o_end = o_col + (want_c ? row : 0);
  if (!h->work.ensure(o_counts + sizeof(int32_t) * (size_t)std::max<int64_t>(nb, 1) * kStsdfCols) || !h->out.ensure(o_end) ||
      !h->back.ensure(o_end))
    return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (scalable TSDF extraction buffers)");
  hipStream_t s = h->stream;
  int64_t* offsets = h->work.as<int64_t>();
  int32_t* totals = reinterpret_cast<int32_t*>(h->work.as<char>() + o_totals);
  int32_t* counts = reinterpret_cast<int32_t*>(h->work.as<char>() + o_counts);
  char* out = h->out.as<char>();
  launch_stsdf_count(s, h->g, d, mode, counts, totals, offsets);
  FCHK(h, hipMemcpyAsync(out, offsets + nb, sizeof(int64_t), hipMemcpyDeviceToDevice, s), "hipMemcpyAsync (count)");
  if (cap > 0)
    launch_stsdf_write(s, h->g, h->ul, d, mode, counts, offsets, cap, reinterpret_cast<double*>(out + o_pts),
                       want_n ? reinterpret_cast<double*>(out + o_norm) : nullptr,
                       want_c ? reinterpret_cast<double*>(out + o_col) : nullptr);
  FCHK(h, hipGetLastError(), "kernel launch (scalable TSDF extraction)");
  FCHK(h, hipMemcpyAsync(h->back.p, out, cap > 0 ? o_end : sizeof(int64_t), hipMemcpyDeviceToHost, s),
       "hipMemcpyAsync (scalable TSDF extraction)");
  FCHK(h, hipStreamSynchronize(s), "scalable TSDF extraction");
  const char* back = h->back.as<char>();
  int64_t count = 0;
  memcpy(&count, back, sizeof(count));
  *count_out = count;
  if (capacity == 0 && !points) return TEASER_HIP_OK;  // the count alone
  if (count > capacity)
    return fail(h, TEASER_HIP_ERR_BAD_ARG,
                "capacity " + std::to_string(capacity) + " is below the count " + std::to_string(count));
  const size_t bytes = sizeof(double) * 3 * (size_t)count;
  if (bytes > 0) {
    memcpy(points, back + o_pts, bytes);
    if (want_n) memcpy(normals, back + o_norm, bytes);
    if (want_c) memcpy(colors, back + o_col, bytes);
  }
  return TEASER_HIP_OK;
}

}  // namespace

extern "C" {

int32_t teaser_hip_stsdf_volume_default(teaser_stsdf_volume_c* v) {
  if (!v) return TEASER_HIP_ERR_BAD_ARG;
  memset(v, 0, sizeof(*v));
  v->voxel_length = 4.0 / 512.0;
  v->sdf_trunc = 0.04;
  v->volume_unit_resolution = kStsdfU;
  v->depth_sampling_stride = 4;
  v->initial_blocks = 1024;
  v->slab_blocks = 1024;
  return TEASER_HIP_OK;
}

int32_t teaser_hip_stsdf_create(const teaser_stsdf_volume_c* vol, int32_t device, teaser_hip_stsdf** out) {
  g_stsdf_create_error.clear();
  if (!out) return refuse_stsdf_create("out must not be NULL");
  *out = nullptr;
  if (!vol) return refuse_stsdf_create("volume must not be NULL");
  const int U = vol->volume_unit_resolution;
  if (U != 4 && U != 8 && U != 16 && U != 32)
    return refuse_stsdf_create("volume_unit_resolution must be a power of two in [4, 32]");
  if (U != kStsdfU) return refuse_stsdf_create("volume_unit_resolution: this version supports only 16");
  if (!std::isfinite(vol->voxel_length) || !(vol->voxel_length > 0.0))
    return refuse_stsdf_create("voxel_length must be finite and > 0");
  const double ul = vol->voxel_length * (double)U;
  if (!std::isfinite(ul)) return refuse_stsdf_create("voxel_length must be finite and > 0");
  if (!std::isfinite(vol->sdf_trunc) || !(vol->sdf_trunc > 0.0)) return refuse_stsdf_create("sdf_trunc must be finite and > 0");
  if (vol->sdf_trunc > ul) return refuse_stsdf_create("sdf_trunc must not exceed a block's side, voxel_length x 16");
  if (vol->color_type < 0 || vol->color_type > 2)
    return refuse_stsdf_create("color_type must be 0 (none), 1 (RGB8) or 2 (Gray32)");
  if (vol->depth_sampling_stride < 1) return refuse_stsdf_create("depth_sampling_stride must be >= 1");
  if (vol->initial_blocks < 1 || vol->slab_blocks < 1) return refuse_stsdf_create("initial_blocks and slab_blocks must be >= 1");
  if (vol->max_blocks < 0) return refuse_stsdf_create("max_blocks must be >= 0");
  if (vol->reserved != 0 || vol->reserved32 != 0) return refuse_stsdf_create("reserved must be 0");
  teaser_hip_stsdf* h = nullptr;
  const int32_t rc = open_handle(device, &h);
  if (rc != TEASER_HIP_OK) return rc;
  h->vol = *vol;
  h->ul = ul;
  TsdfGrid& g = h->g;
  memset(&g, 0, sizeof(g));
  g.R = U, g.color_type = vol->color_type;
  g.vl = ul / (double)U;  // as the dense volume forms it from length = ul: voxel_length again
  g.half = g.vl * 0.5;
  g.vl_f = (float)g.vl;
  g.half_f = g.vl_f * 0.5f;
  g.trunc_f = (float)vol->sdf_trunc;
  g.inv_f = 1.0f / g.trunc_f;
  h->block_bytes = (size_t)(g.color_type != 0 ? 32 : 8) * kStsdfVoxels;
  *out = h;
  return TEASER_HIP_OK;
}

int32_t teaser_hip_stsdf_destroy(teaser_hip_stsdf* h) { return close_handle(h); }
const char* teaser_hip_stsdf_last_error(const teaser_hip_stsdf* h) {
  return h ? h->err.c_str() : g_stsdf_create_error.c_str();
}

int32_t teaser_hip_stsdf_fill_scratch(teaser_hip_stsdf* h, int32_t byte, int64_t* bytes_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  // not the slabs and not h->dir: the blocks and the directory are the handle's state
  const ScratchSpan spans[] = {span_of(h->in),    span_of(h->work), span_of(h->out),    span_of(h->items),
                               span_of(h->stage), span_of(h->back), span_of(h->istage), span_of(h->mesh)};
  return fill_scratch(h, byte, spans, 8, bytes_out);
}

int32_t teaser_hip_stsdf_last_phases(const teaser_hip_stsdf* h, double* ms) {
  if (!h || !ms) return TEASER_HIP_ERR_BAD_ARG;
  for (int k = 0; k < 3; ++k) ms[k] = h->phase_ms[k];
  return TEASER_HIP_OK;
}

int32_t teaser_hip_stsdf_reset(teaser_hip_stsdf* h) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  h->keys.clear();  // the slabs stay: a block is zeroed when it is opened
  h->slots.clear();
  h->dir_dirty = true;
  return TEASER_HIP_OK;
}

int32_t teaser_hip_stsdf_integrate_frames(teaser_hip_stsdf* h, int32_t n_frames, const teaser_tsdf_frame_c* frames,
                                          const void* const* depth, const void* const* color, int64_t* touched_out,
                                          int64_t* opened_out, int64_t* out_of_range_out) {
  return integrate(h, n_frames, frames, depth, color, touched_out, opened_out, out_of_range_out);
}

int32_t teaser_hip_stsdf_extract_point_cloud(teaser_hip_stsdf* h, int64_t capacity, double* points, double* normals,
                                             double* colors, int64_t* count_out) {
  return extract(h, 0, capacity, points, normals, colors, count_out);
}

int32_t teaser_hip_stsdf_extract_voxel_point_cloud(teaser_hip_stsdf* h, int64_t capacity, double* points, double* colors,
                                                   int64_t* count_out) {
  return extract(h, 1, capacity, points, nullptr, colors, count_out);
}

int32_t teaser_hip_stsdf_block_count(teaser_hip_stsdf* h, int64_t* count_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (!count_out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "count_out must not be NULL");
  *count_out = (int64_t)h->keys.size();
  return TEASER_HIP_OK;
}

int32_t teaser_hip_stsdf_block_keys(teaser_hip_stsdf* h, int64_t capacity, int32_t* keys, int64_t* count_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (!count_out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "count_out must not be NULL");
  if (capacity < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "capacity must be >= 0");
  if (capacity > 0 && !keys) return fail(h, TEASER_HIP_ERR_BAD_ARG, "keys must not be NULL with a capacity above 0");
  const int64_t n = (int64_t)h->keys.size();
  *count_out = n;
  if (capacity == 0 && !keys) return TEASER_HIP_OK;
  if (n > capacity)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "capacity " + std::to_string(capacity) + " is below the count " + std::to_string(n));
  for (int64_t k = 0; k < n; ++k) stsdf_unkey(h->keys[(size_t)k], keys + 3 * k);
  return TEASER_HIP_OK;
}

int32_t teaser_hip_stsdf_download_blocks(teaser_hip_stsdf* h, int64_t capacity, float* tsdf_weight, double* color,
                                         int64_t* count_out) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (!count_out) return fail(h, TEASER_HIP_ERR_BAD_ARG, "count_out must not be NULL");
  if (capacity < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "capacity must be >= 0");
  const int64_t n = (int64_t)h->keys.size();
  *count_out = n;
  if (capacity == 0 && !tsdf_weight && !color) return TEASER_HIP_OK;
  if (!tsdf_weight && !color) return fail(h, TEASER_HIP_ERR_BAD_ARG, "tsdf_weight and color are both NULL");
  if (color && h->g.color_type == 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "color is given for a volume without colour");
  if (n > capacity)
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "capacity " + std::to_string(capacity) + " is below the count " + std::to_string(n));
  if (n == 0) return TEASER_HIP_OK;
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  StsdfDir d;
  const int32_t rc = stsdf_sync_directory(h, &d);
  if (rc != TEASER_HIP_OK) return rc;
  const size_t per_tw = 8 * (size_t)kStsdfVoxels, per_c = 24 * (size_t)kStsdfVoxels;
  if (!h->out.ensure((color ? per_c : per_tw) * (size_t)std::min<int64_t>(n, kBatchBlocks)))
    return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (block download buffer)");
  hipStream_t s = h->stream;
  for (int64_t b0 = 0; b0 < n; b0 += kBatchBlocks) {  // the one buffer serves every step, in stream order
    const int cnt = (int)std::min<int64_t>(kBatchBlocks, n - b0);
    if (tsdf_weight) {
      launch_stsdf_export(s, h->g.color_type, d.base + b0, cnt, h->out.as<float>(), nullptr);
      FCHK(h, hipMemcpyAsync(tsdf_weight + 2 * (size_t)kStsdfVoxels * (size_t)b0, h->out.p, per_tw * (size_t)cnt,
                             hipMemcpyDeviceToHost, s), "hipMemcpyAsync (block download)");
    }
    if (color) {
      launch_stsdf_export(s, h->g.color_type, d.base + b0, cnt, nullptr, h->out.as<double>());
      FCHK(h, hipMemcpyAsync(color + 3 * (size_t)kStsdfVoxels * (size_t)b0, h->out.p, per_c * (size_t)cnt,
                             hipMemcpyDeviceToHost, s), "hipMemcpyAsync (block download)");
    }
  }
  FCHK(h, hipGetLastError(), "kernel launch (block download)");
  FCHK(h, hipStreamSynchronize(s), "block download");
  return TEASER_HIP_OK;
}

int32_t teaser_hip_stsdf_upload_blocks(teaser_hip_stsdf* h, int64_t n_blocks, const int32_t* keys, const float* tsdf_weight,
                                       const double* color) {
  if (!h) return TEASER_HIP_ERR_BAD_ARG;
  h->err.clear();
  if (n_blocks < 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_blocks must be >= 0");
  if (n_blocks == 0) return TEASER_HIP_OK;
  if (!keys) return fail(h, TEASER_HIP_ERR_BAD_ARG, "keys must not be NULL");
  if (!tsdf_weight && !color) return fail(h, TEASER_HIP_ERR_BAD_ARG, "tsdf_weight and color are both NULL");
  if (color && h->g.color_type == 0) return fail(h, TEASER_HIP_ERR_BAD_ARG, "color is given for a volume without colour");
  if (n_blocks > INT32_MAX) return fail(h, TEASER_HIP_ERR_BAD_ARG, "n_blocks is above 2^31 - 1");
  const size_t n = (size_t)n_blocks;
  std::vector<uint64_t> given(n);
  for (size_t k = 0; k < n; ++k) {
    for (int a = 0; a < 3; ++a)
      if (keys[3 * k + a] < -kStsdfBias || keys[3 * k + a] >= kStsdfBias)
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "keys: an index outside [-2^20, 2^20) (block " + std::to_string(k) + ")");
    given[k] = stsdf_key(keys[3 * k], keys[3 * k + 1], keys[3 * k + 2]);
  }
  std::vector<uint64_t> sorted = given;
  std::sort(sorted.begin(), sorted.end());
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
    return fail(h, TEASER_HIP_ERR_BAD_ARG, "keys: a block occurs twice");
  if (tsdf_weight)
    for (size_t k = 0; k < 2 * n * kStsdfVoxels; ++k)
      if (!std::isfinite(tsdf_weight[k])) return fail(h, TEASER_HIP_ERR_BAD_ARG, "tsdf_weight has a non-finite value");
  if (color)
    for (size_t k = 0; k < 3 * n * kStsdfVoxels; ++k)
      if (!std::isfinite(color[k]) && !(h->g.color_type == 2 && std::isnan(color[k])))  // Gray32 may hold NaN
        return fail(h, TEASER_HIP_ERR_BAD_ARG, "color has a non-finite value");
  std::vector<uint64_t> fresh;
  for (uint64_t key : sorted)
    if (!std::binary_search(h->keys.begin(), h->keys.end(), key)) fresh.push_back(key);
  FCHK(h, hipSetDevice(h->device), "hipSetDevice");
  const size_t per_tw = 8 * (size_t)kStsdfVoxels, per_c = 24 * (size_t)kStsdfVoxels;
  if (!h->out.ensure((color ? per_c : per_tw) * std::min<size_t>(n, kBatchBlocks)) || !h->items.ensure(sizeof(char*) * n) ||
      !h->istage.ensure(sizeof(char*) * n))
    return fail(h, TEASER_HIP_ERR_OOM, "allocation failed (block upload buffers)");
  const int32_t rc = open_blocks(h, fresh);
  if (rc != TEASER_HIP_OK) return rc;
  char** base = h->istage.as<char*>();
  for (size_t k = 0; k < n; ++k) {
    const size_t e = (size_t)(std::lower_bound(h->keys.begin(), h->keys.end(), given[k]) - h->keys.begin());
    base[k] = stsdf_block_ptr(h, h->slots[e]);
  }
  hipStream_t s = h->stream;
  FCHK(h, hipMemcpyAsync(h->items.p, base, sizeof(char*) * n, hipMemcpyHostToDevice, s), "hipMemcpyAsync (block upload)");
  char* const* d_base = h->items.as<char*>();
  for (size_t b0 = 0; b0 < n; b0 += kBatchBlocks) {
    const int cnt = (int)std::min<size_t>(kBatchBlocks, n - b0);
    if (tsdf_weight) {
      FCHK(h, hipMemcpyAsync(h->out.p, tsdf_weight + 2 * (size_t)kStsdfVoxels * b0, per_tw * (size_t)cnt,
                             hipMemcpyHostToDevice, s), "hipMemcpyAsync (block upload)");
      launch_stsdf_import(s, h->g.color_type, d_base + b0, cnt, h->out.as<float>(), nullptr);
    }
    if (color) {
      FCHK(h, hipMemcpyAsync(h->out.p, color + 3 * (size_t)kStsdfVoxels * b0, per_c * (size_t)cnt, hipMemcpyHostToDevice, s),
           "hipMemcpyAsync (block upload)");
      launch_stsdf_import(s, h->g.color_type, d_base + b0, cnt, nullptr, h->out.as<double>());
    }
  }
  FCHK(h, hipGetLastError(), "kernel launch (block upload)");
  FCHK(h, hipStreamSynchronize(s), "block upload");
  return TEASER_HIP_OK;
}

}  // extern "C"
