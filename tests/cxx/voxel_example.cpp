// teaser::VoxelGrid (include/teaser/voxel.h) used like Open3D's pcd.voxel_down_sample.
//   voxel_example            a small cloud with hand-computed voxels; 0 ok, 1 wrong result
//   voxel_example DIR v      reads DIR/points.bin (n x 3 doubles), down-samples at voxel size v, writes
//                            DIR/means.bin (n_out x 3 doubles), DIR/counts.bin and DIR/trace.bin (int32), prints n_out
// Exit code 77: no MI355X visible (loud failure, no CPU path); 1: any other failure.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "teaser/voxel.h"

static std::vector<double> read_doubles(const std::string& path) {
  std::vector<double> v;
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return v;
  double x;
  while (std::fread(&x, sizeof(double), 1, f) == 1) v.push_back(x);
  std::fclose(f);
  return v;
}

static bool write_bytes(const std::string& path, const void* p, size_t bytes) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes;
  return std::fclose(f) == 0 && ok;
}

static teaser::Matrix3X cloud(const std::vector<double>& xyz) {
  teaser::Matrix3X m(3, (int64_t)(xyz.size() / 3));
  for (int64_t i = 0; i < m.cols(); ++i)
    for (int r = 0; r < 3; ++r) m(r, i) = xyz[(size_t)(3 * i + r)];
  return m;
}

int main(int argc, char** argv) {
  try {
    teaser::VoxelGrid grid;
    if (argc == 3) {
      const std::string dir = argv[1];
      const teaser::VoxelDownSampleResult res =
          grid.voxelDownSample(cloud(read_doubles(dir + "/points.bin")), std::atof(argv[2]), true);
      const int64_t m = res.points.cols();
      std::vector<double> means((size_t)(3 * m));
      for (int64_t k = 0; k < m; ++k)
        for (int r = 0; r < 3; ++r) means[(size_t)(3 * k + r)] = res.points(r, k);
      if (!write_bytes(dir + "/means.bin", means.data(), 8 * means.size()) ||
          !write_bytes(dir + "/counts.bin", res.counts.data(), 4 * res.counts.size()) ||
          !write_bytes(dir + "/trace.bin", res.voxel_of_point.data(), 4 * res.voxel_of_point.size()))
        return 1;
      std::printf("n_out %lld\n", (long long)m);
      return 0;
    }
    // voxel size 1, min_bound (0, 0, 0) -> lo = (-0.5, -0.5, -0.5): points 0 and 2 share voxel (0, 0, 0), point 3
    // lies in voxel (0, 0, 1) and sorts after it, point 1 in (2, 0, 0) and sorts last
    const teaser::Matrix3X m =
        teaser::voxelDownSample(cloud({0, 0, 0, 1.5, 0, 0, 0.25, 0.25, 0.25, 0, 0, 1.0}), 1.0);
    const bool ok = m.cols() == 3 && m(0, 0) == 0.125 && m(1, 0) == 0.125 && m(2, 0) == 0.125 && m(2, 1) == 1.0 &&
                    m(0, 2) == 1.5;
    std::printf("%lld voxels\n", (long long)m.cols());
    return ok ? 0 : 1;
  } catch (const teaser::VoxelError& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status() == TEASER_HIP_ERR_NO_DEVICE ? 77 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
