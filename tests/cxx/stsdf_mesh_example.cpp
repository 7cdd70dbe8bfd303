// teaser::ScalableTSDFVolume::extractTriangleMesh (include/teaser/tsdf.h) and teaser::PLYWriter::writeMesh
// (include/teaser/ply_io.h) used like Open3D's extract_triangle_mesh and write_triangle_mesh.  The frames are those of
// tests/cxx/stsdf_example.cpp (tests/test_gpu_tsdf_cxx.py builds the same arrays).  The record printed -- counts and
// FNV-1a hashes of the bytes of every output -- is what tests/test_gpu_stsdf_mesh_cxx.py compares with the Python calls';
// the mesh is written to argv[1] (binary PLY) and argv[2] (ascii PLY).
// Exit code: 0 ok, 77 no MI355X visible (loud failure, no CPU path), 1 wrong result.
#include <cstdio>
#include <cstring>
#include <vector>

#include "teaser/ply_io.h"
#include "teaser/tsdf.h"

static int fail(const char* what) {
  std::fprintf(stderr, "stsdf_mesh_example: %s\n", what);
  return 1;
}

static unsigned long long fnv(const void* p, size_t bytes) {
  unsigned long long h = 1469598103934665603ull;
  const unsigned char* b = (const unsigned char*)p;
  for (size_t k = 0; k < bytes; ++k) h = (h ^ b[k]) * 1099511628211ull;
  return h;
}

int main(int argc, char** argv) {
  if (argc != 3) return fail("usage: stsdf_mesh_example BINARY.ply ASCII.ply");
  try {
    const int w = 40, h = 30, padded = 44;  // the depth rows lie 44 samples apart
    std::vector<std::vector<uint16_t>> depth(2, std::vector<uint16_t>((size_t)(padded * h), 9));
    std::vector<std::vector<uint8_t>> rgb(2, std::vector<uint8_t>((size_t)(3 * w * h)));
    for (int k = 0; k < 2; ++k)
      for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j) {
          depth[k][(size_t)(padded * i + j)] = (uint16_t)((i * 7 + j * 13) % 50 == 0 ? 0 : 900 + 4 * i + 3 * j + 20 * k + (i * j) % 7);
          uint8_t* px = &rgb[k][(size_t)(3 * (w * i + j))];
          px[0] = (uint8_t)((i * 3 + j + 40 * k) % 256), px[1] = (uint8_t)((i + j * 5) % 256), px[2] = (uint8_t)((i * j + k) % 256);
        }
    const teaser::PinholeCameraIntrinsic K(w, h, 32.0, 32.0, 19.5, 14.5);
    std::vector<teaser::Matrix4> E(2, teaser::Matrix4::Identity());  // world to camera
    E[1](0, 3) = 0.0625, E[1](1, 3) = -0.03125, E[1](2, 3) = 0.015625;
    std::vector<teaser::DepthFrame> frames;
    for (int k = 0; k < 2; ++k) {
      frames.push_back(teaser::DepthFrame::U16(depth[k].data(), w, h, 2 * padded));
      frames.back().withRGB8(rgb[k].data());
    }

    teaser::ScalableTSDFVolume vol(0.0625, 0.15, teaser::TSDFVolumeColorType::RGB8, 16, 1);
    const teaser::TSDFTriangleMesh none = vol.extractTriangleMesh(true);
    if (none.vertices.cols() != 0 || !none.triangles.empty()) return fail("a fresh volume has no mesh");
    vol.integrateBatch(frames, {K}, E);
    if (vol.blockCount() <= 1) return fail("more than one block");
    const teaser::TSDFTriangleMesh mesh = vol.extractTriangleMesh(true);
    const int64_t nv = mesh.vertices.cols();
    const size_t nt = mesh.triangles.size() / 3;
    if (nv <= 0 || nt == 0 || mesh.triangles.size() != 3 * nt) return fail("the mesh has rows");
    if (mesh.vertex_colors.cols() != nv || mesh.vertex_normals.cols() != nv) return fail("a colour and a normal per vertex");
    for (int32_t t : mesh.triangles)
      if (t < 0 || t >= nv) return fail("a triangle index outside the vertices");
    const teaser::TSDFTriangleMesh plain = vol.extractTriangleMesh();
    const size_t bytes = sizeof(double) * 3 * (size_t)nv;
    if (plain.vertex_normals.cols() != 0 || plain.vertices.cols() != nv || plain.triangles != mesh.triangles ||
        std::memcmp(plain.vertices.data(), mesh.vertices.data(), bytes) != 0)
      return fail("without normals the same mesh");
    teaser::ScalableTSDFVolume bare(0.0625, 0.15, teaser::TSDFVolumeColorType::NoColor, 16, 1);
    bare.integrateBatch(frames, {K}, E);
    const teaser::TSDFTriangleMesh grey = bare.extractTriangleMesh();
    if (grey.vertex_colors.cols() != 0 || grey.triangles != mesh.triangles) return fail("a volume without colour gives the same triangles");
    bare.reset();
    if (!bare.extractTriangleMesh().triangles.empty()) return fail("reset closes every block");

    teaser::PLYWriter writer;
    if (writer.writeMesh(argv[1], mesh.vertices, mesh.vertex_colors, mesh.triangles) != 0) return fail("the binary PLY");
    if (writer.writeMesh(argv[2], mesh.vertices, mesh.vertex_colors, mesh.triangles, false) != 0) return fail("the ascii PLY");
    teaser::PointCloud back;  // the reader of this header skips the colours and the faces
    if (teaser::PLYReader().read(argv[1], back) != 0 || (int64_t)back.size() != nv) return fail("the PLY reads back");

    std::printf("blocks %lld\nvertices %lld\ntriangles %lld\n", (long long)vol.blockCount(), (long long)nv, (long long)nt);
    std::printf("vertex_bits %016llx\ncolor_bits %016llx\nnormal_bits %016llx\ntriangle_bits %016llx\n", fnv(mesh.vertices.data(), bytes),
                fnv(mesh.vertex_colors.data(), bytes), fnv(mesh.vertex_normals.data(), bytes),
                fnv(mesh.triangles.data(), sizeof(int32_t) * mesh.triangles.size()));
    std::printf("checks 1\n");
    return 0;
  } catch (const teaser::TSDFError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
