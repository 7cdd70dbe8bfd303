// Host-only check of the triangle mesh of the TSDF volume (tests/test_tsdf_mesh_host.py): csrc/tsdf.hip and
// csrc/tsdf_mesh.hip compiled by g++ against the HIP stand-in header (tests/hip_stub), built with -ffp-contract=off
// -fsanitize=address,undefined as a stand-alone program.  The volume's launchers, the reader of the case file and the
// helpers are those of tests/tsdf_host_driver.cpp, which is included with its main renamed (its cases are not run here);
// the mesh's launchers are serial loops over the column functions of csrc/tsdf_mesh_device.h -- the text the kernels
// compile.  "Device" buffers are host allocations of the size the host code asked for, so a scratch or output layout
// that is sized or addressed wrongly is an AddressSanitizer report.  Counts, vertices, colours, normals and triangles are
// compared for equality with those of tests/tsdf_mesh_reference.py, read from a text file (hexadecimal floats).
//   tsdf_mesh_host_driver CASES.txt    exit code 0: every case equal and every refusal refused
// TEST INFRASTRUCTURE ONLY.
#define main tsdf_host_driver_main
#include "tsdf_host_driver.cpp"
#undef main
#include "../teaser-plusplus_amd/csrc/tsdf_mesh.hip"

static int g_mesh_launches = 0;

namespace thip {

void launch_tsdf_mesh_cubes(hipStream_t, const TsdfGrid& g, const TsdfFields& v, unsigned char* cubes) {
  ++g_mesh_launches;
  for (int x = 0; x < g.R; ++x)
    for (int y = 0; y < g.R; ++y) tsdf_mesh_column_cubes(g, v, x, y, cubes);
}

void launch_tsdf_mesh_count(hipStream_t, const TsdfGrid& g, const unsigned char* cubes, uint32_t* records, int32_t* counts,
                            int64_t* offsets, int64_t* totals) {
  g_mesh_launches += 2;
  const int64_t plane = (int64_t)g.R * g.R;
  for (int x = 0; x < g.R; ++x)
    for (int y = 0; y < g.R; ++y) {
      const int64_t col = (int64_t)x * g.R + y;
      tsdf_mesh_column_count(cubes, g.R, x, y, records, &counts[col], &counts[plane + col]);
      if (counts[col] < 0 || counts[col] > 12 * (g.R - 1) || counts[plane + col] > 5 * (g.R - 1)) std::abort();
    }
  for (int a = 0; a < 2; ++a) {
    int64_t run = 0;
    for (int64_t col = 0; col < plane; ++col) {
      offsets[a * (plane + 1) + col] = run;
      run += counts[a * plane + col];
    }
    offsets[a * (plane + 1) + plane] = totals[a] = run;
  }
}

void launch_tsdf_mesh_vertices(hipStream_t, const TsdfGrid& g, const TsdfFields& v, const unsigned char* cubes,
                               const uint32_t* records, const int64_t* offsets, const int64_t* totals, int64_t vertex_capacity,
                               int64_t triangle_capacity, double* vertices, double* colors, double* normals) {
  ++g_mesh_launches;
  if (!tsdf_mesh_fits(totals, vertex_capacity, triangle_capacity)) return;
  for (int x = 0; x < g.R; ++x)
    for (int y = 0; y < g.R; ++y) tsdf_mesh_column_vertices(g, v, cubes, records, offsets, x, y, vertices, colors, normals);
}

void launch_tsdf_mesh_triangles(hipStream_t, const TsdfGrid& g, const unsigned char* cubes, const uint32_t* records,
                                const int64_t* offsets, const int64_t* totals, int64_t vertex_capacity,
                                int64_t triangle_capacity, int32_t* triangles) {
  ++g_mesh_launches;
  if (!tsdf_mesh_fits(totals, vertex_capacity, triangle_capacity)) return;
  const int64_t plane = (int64_t)g.R * g.R;
  for (int x = 0; x < g.R; ++x)
    for (int y = 0; y < g.R; ++y)
      tsdf_mesh_column_triangles(cubes, records, offsets, offsets + plane + 1, g.R, x, y, triangles);
}

}  // namespace thip

struct MeshCase {
  teaser_tsdf_volume_c vol;
  std::vector<float> tw;
  std::vector<double> color, vert, col, nrm;
  std::vector<int32_t> tri;
  int64_t nv = 0, nt = 0;
};

// The counts alone, the exact capacities, room to spare, one row too few in either array, and a second call.
static void check_mesh(teaser_hip_tsdf* h, const MeshCase& cs, int c) {
  const bool colored = cs.vol.color_type != 0;
  int64_t nv = -5, nt = -5;
  g_mesh_launches = 0;
  expect(teaser_hip_tsdf_extract_triangle_mesh(h, 0, nullptr, nullptr, nullptr, 0, nullptr, &nv, &nt) == TEASER_HIP_OK &&
             nv == cs.nv && nt == cs.nt, "the counts alone", c);
  expect(g_mesh_launches == 3, "three launches for the counts", c);
  if (nv != cs.nv || nt != cs.nt) return;
  const size_t n = (size_t)nv, m = (size_t)nt;
  std::vector<double> p(3 * n + 3, -7.5), cc(3 * n + 3, -7.5), nn(3 * n + 3, -7.5);
  std::vector<int32_t> t(3 * m + 3, -7);
  nv = nt = -5;
  g_mesh_launches = 0;
  expect(teaser_hip_tsdf_extract_triangle_mesh(h, (int64_t)n, p.data(), colored ? cc.data() : nullptr, nn.data(), (int64_t)m,
                                               t.data(), &nv, &nt) == TEASER_HIP_OK && nv == cs.nv && nt == cs.nt,
         "extraction with the exact capacities", c);
  expect(g_mesh_launches == 3 + (n > 0) + (m > 0), "one launch more per array", c);
  for (size_t k = 3 * n; k < 3 * n + 3; ++k) expect(p[k] == -7.5 && cc[k] == -7.5 && nn[k] == -7.5, "a vertex row behind the count is written", c);
  for (size_t k = 3 * m; k < 3 * m + 3; ++k) expect(t[k] == -7, "a triangle row behind the count is written", c);
  p.resize(3 * n), cc.resize(3 * n), nn.resize(3 * n), t.resize(3 * m);
  expect(same(p, cs.vert), "vertex bits", c);
  expect(same(nn, cs.nrm), "vertex normal bits", c);
  if (colored) expect(same(cc, cs.col), "vertex colour bits", c);
  expect(same(t, cs.tri), "triangle rows", c);
  if (n == 0 || m == 0) return;
  // room to spare and no optional output
  std::vector<double> big(3 * (n + 50), -7.5);
  std::vector<int32_t> tbig(3 * (m + 70), -7);
  expect(teaser_hip_tsdf_extract_triangle_mesh(h, (int64_t)n + 50, big.data(), nullptr, nullptr, (int64_t)m + 70, tbig.data(), &nv,
                                               &nt) == TEASER_HIP_OK, "extraction with room to spare", c);
  expect(big[3 * n] == -7.5 && tbig[3 * m] == -7, "room to spare: rows behind the counts", c);
  big.resize(3 * n), tbig.resize(3 * m);
  expect(same(big, cs.vert) && same(tbig, cs.tri), "bits with room to spare", c);
  // one row too few, in either array: refused, both counts named and reported, nothing written to either
  for (int which = 0; which < 2; ++which) {
    std::vector<double> q(3 * n, -7.5), qn(3 * n, -7.5);
    std::vector<int32_t> qt(3 * m, -7);
    nv = nt = -5;
    refused(h, teaser_hip_tsdf_extract_triangle_mesh(h, (int64_t)n - (which == 0), q.data(), nullptr, qn.data(),
                                                     (int64_t)m - (which == 1), qt.data(), &nv, &nt),
            ("vertex count " + std::to_string(n)).c_str(), ("triangle count " + std::to_string(m)).c_str());
    expect(nv == cs.nv && nt == cs.nt, "the refused extraction reports the counts", c);
    expect(q == std::vector<double>(3 * n, -7.5) && qn == q && qt == std::vector<int32_t>(3 * m, -7),
           "the refused extraction writes nothing", c);
  }
  // vertices alone cannot be had: the triangle capacity 0 is below the count
  std::vector<double> q(3 * n, -7.5);
  refused(h, teaser_hip_tsdf_extract_triangle_mesh(h, (int64_t)n, q.data(), nullptr, nullptr, 0, nullptr, &nv, &nt),
          "triangle_capacity 0", "below its count");
  expect(q == std::vector<double>(3 * n, -7.5), "vertices alone: nothing written", c);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const int nc = (int)read_number(f);
  std::vector<MeshCase> cases((size_t)nc);
  for (MeshCase& cs : cases) {
    if (teaser_hip_tsdf_volume_default(&cs.vol) != TEASER_HIP_OK) return 2;
    cs.vol.resolution = (int)read_number(f), cs.vol.color_type = (int)read_number(f);
    cs.vol.length = read_number(f), cs.vol.sdf_trunc = read_number(f);
    for (double& o : cs.vol.origin) o = read_number(f);
    const size_t n = (size_t)cs.vol.resolution * cs.vol.resolution * cs.vol.resolution;
    read_numbers(f, cs.tw, 2 * n);
    if (cs.vol.color_type) read_numbers(f, cs.color, 3 * n);
    cs.nv = (int64_t)read_number(f);
    read_numbers(f, cs.vert, 3 * (size_t)cs.nv);
    read_numbers(f, cs.nrm, 3 * (size_t)cs.nv);
    if (cs.vol.color_type) read_numbers(f, cs.col, 3 * (size_t)cs.nv);
    cs.nt = (int64_t)read_number(f);
    read_numbers(f, cs.tri, 3 * (size_t)cs.nt);
  }
  std::fclose(f);

  const MeshCase* plain = nullptr;
  for (int c = 0; c < nc; ++c) {
    const MeshCase& cs = cases[(size_t)c];
    if (cs.vol.color_type == 0 && cs.nv > 0) plain = &cs;
    teaser_hip_tsdf* h = nullptr;
    if (teaser_hip_tsdf_create(&cs.vol, 0, &h) != TEASER_HIP_OK) return 2;
    int64_t nv = -5, nt = -5;
    expect(teaser_hip_tsdf_extract_triangle_mesh(h, 0, nullptr, nullptr, nullptr, 0, nullptr, &nv, &nt) == TEASER_HIP_OK && nv == 0 &&
               nt == 0, "an empty volume has no mesh", c);
    expect(teaser_hip_tsdf_upload(h, cs.tw.data(), cs.vol.color_type ? cs.color.data() : nullptr) == TEASER_HIP_OK, "upload", c);
    check_mesh(h, cs, c);
    // the point cloud between two meshes: the scratch of one does not disturb the other or the volume
    int64_t before = -5, after = -5;
    expect(teaser_hip_tsdf_extract_point_cloud(h, 0, nullptr, nullptr, nullptr, &before) == TEASER_HIP_OK, "point cloud", c);
    check_mesh(h, cs, c);
    expect(teaser_hip_tsdf_extract_point_cloud(h, 0, nullptr, nullptr, nullptr, &after) == TEASER_HIP_OK && after == before,
           "the point cloud after the mesh", c);
    std::vector<float> tw(cs.tw.size(), -7.5f);
    expect(teaser_hip_tsdf_download(h, tw.data(), nullptr) == TEASER_HIP_OK && same(tw, cs.tw), "the mesh leaves the volume alone", c);
    teaser_hip_tsdf_destroy(h);
  }

  // refusals: BAD_ARG with the argument named; the handle stays usable
  if (!plain) return 2;
  {
    const MeshCase& cs = *plain;
    teaser_hip_tsdf* h = nullptr;
    if (teaser_hip_tsdf_create(&cs.vol, 0, &h) != TEASER_HIP_OK) return 2;
    if (teaser_hip_tsdf_upload(h, cs.tw.data(), nullptr) != TEASER_HIP_OK) return 2;
    int64_t nv = 0, nt = 0;
    std::vector<double> room(3 * (size_t)cs.nv);
    std::vector<int32_t> troom(3 * (size_t)cs.nt);
    refused(h, teaser_hip_tsdf_extract_triangle_mesh(h, cs.nv, room.data(), nullptr, nullptr, cs.nt, troom.data(), nullptr, &nt),
            "vertex_count_out and triangle_count_out", "");
    refused(h, teaser_hip_tsdf_extract_triangle_mesh(h, cs.nv, room.data(), nullptr, nullptr, cs.nt, troom.data(), &nv, nullptr),
            "vertex_count_out and triangle_count_out", "");
    refused(h, teaser_hip_tsdf_extract_triangle_mesh(h, -1, room.data(), nullptr, nullptr, cs.nt, troom.data(), &nv, &nt),
            "vertex_capacity must be >= 0", "");
    refused(h, teaser_hip_tsdf_extract_triangle_mesh(h, cs.nv, room.data(), nullptr, nullptr, -1, troom.data(), &nv, &nt),
            "triangle_capacity must be >= 0", "");
    refused(h, teaser_hip_tsdf_extract_triangle_mesh(h, cs.nv, nullptr, nullptr, nullptr, cs.nt, troom.data(), &nv, &nt),
            "vertices must not be NULL", "");
    refused(h, teaser_hip_tsdf_extract_triangle_mesh(h, cs.nv, room.data(), nullptr, nullptr, cs.nt, nullptr, &nv, &nt),
            "triangles must not be NULL", "");
    refused(h, teaser_hip_tsdf_extract_triangle_mesh(h, cs.nv, room.data(), room.data(), nullptr, cs.nt, troom.data(), &nv, &nt),
            "vertex_colors is given for a volume without colour", "");
    expect(teaser_hip_tsdf_extract_triangle_mesh(nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, &nv, &nt) == TEASER_HIP_ERR_BAD_ARG,
           "refusal: NULL handle", -1);
    check_mesh(h, cs, -1);  // nothing above left a trace
    teaser_hip_tsdf_destroy(h);
  }
  {
    int32_t edge[256];
    int8_t tri[4096];
    expect(teaser_hip_tsdf_mesh_tables(edge, tri) == TEASER_HIP_OK && edge[1] == 0x109 && edge[3] == 0x30a && tri[16] == 0 &&
               tri[17] == 8 && tri[18] == 3 && tri[19] == -1, "the tables", -1);
    expect(teaser_hip_tsdf_mesh_tables(nullptr, tri) == TEASER_HIP_ERR_BAD_ARG && teaser_hip_tsdf_mesh_tables(edge, nullptr) == TEASER_HIP_ERR_BAD_ARG,
           "refusal: tables NULL", -1);
  }
  std::printf("cases %d  mismatches %d\n", nc, g_bad);
  return g_bad ? 1 : 0;
}
