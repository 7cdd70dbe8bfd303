// teaser::FPFHEstimation::computeFPFHFeaturesBatch and teaser::Matcher::calculateCorrespondencesBatch through the
// drop-in headers: the cloud of argv[1] (ascii PLY, x y z vertices), a transformed noisy copy and an empty cloud in
// ONE call each, compared with the single-cloud / single-pair methods (bit for bit: the batched front-end's contract).
// Exit code: 0 ok, 77 no MI355X visible, 2 unreadable input, 1 wrong result.
#include <cstdio>
#include <cstring>
#include <random>

#include "teaser/fpfh.h"
#include "teaser/matcher.h"
#include "teaser/ply_io.h"

int main(int argc, char** argv) {
  teaser::PointCloud src_cloud;
  if (argc >= 2) {
    teaser::PLYReader reader;
    if (reader.read(argv[1], src_cloud) != 0 || src_cloud.size() < 10) return 2;
  } else {  // a small synthetic surface patch
    std::mt19937 rng(3);
    std::uniform_real_distribution<float> u(0.f, 0.3f);
    for (int i = 0; i < 600; ++i) {
      const float x = u(rng), y = u(rng);
      src_cloud.push_back({x, y, 0.5f * x * x - 0.3f * x * y});
    }
  }
  std::mt19937 rng(7);
  std::uniform_real_distribution<float> noise(-0.0005f, 0.0005f);
  teaser::PointCloud tgt_cloud;
  for (size_t i = 0; i < src_cloud.size(); ++i) {
    const teaser::PointXYZ& p = src_cloud[i];
    tgt_cloud.push_back({p.y + 0.1f + noise(rng), -p.x + noise(rng), p.z - 0.05f + noise(rng)});
  }
  try {
    teaser::FPFHEstimation fpfh;
    const std::vector<teaser::PointCloud> clouds = {src_cloud, tgt_cloud, teaser::PointCloud()};
    const std::vector<teaser::FPFHCloud> feats = fpfh.computeFPFHFeaturesBatch(clouds, 0.02, 0.04);
    const std::vector<teaser::NormalCloud> normals = fpfh.getNormalsBatch();
    bool ok = feats.size() == 3 && normals.size() == 3 && feats[2].empty() && normals[2].empty();
    for (size_t b = 0; ok && b < 2; ++b) {
      const teaser::FPFHCloudPtr one = fpfh.computeFPFHFeatures(clouds[b], 0.02, 0.04);
      const teaser::NormalCloud n1 = fpfh.getNormals();
      ok = one->size() == feats[b].size() && n1.size() == normals[b].size() &&
           std::memcmp(one->data(), feats[b].data(), sizeof(teaser::FPFHSignature33) * one->size()) == 0 &&
           std::memcmp(n1.data(), normals[b].data(), sizeof(teaser::Normal) * n1.size()) == 0;
    }
    teaser::Matcher matcher;
    const std::vector<teaser::FPFHCloud> fs = {feats[0], feats[1], feats[2]}, ft = {feats[1], feats[0], feats[0]};
    const std::vector<teaser::PointCloud> ps = {src_cloud, tgt_cloud, teaser::PointCloud()},
                                          pt = {tgt_cloud, src_cloud, src_cloud};
    const auto corr = matcher.calculateCorrespondencesBatch(ps, pt, fs, ft, false, true, false, 0);
    ok = ok && corr.size() == 3 && corr[2].empty() && !corr[0].empty();
    for (size_t b = 0; ok && b < 2; ++b)
      ok = corr[b] == matcher.calculateCorrespondences(ps[b], pt[b], fs[b], ft[b], false, true, false, 0);
    std::printf("points %zu  correspondences %zu / %zu  batch == single %d\n", src_cloud.size(),
                corr.size() > 0 ? corr[0].size() : 0, corr.size() > 1 ? corr[1].size() : 0, (int)ok);
    return ok ? 0 : 1;
  } catch (const std::runtime_error& e) {
    std::printf("facade: %s\n", e.what());
    return 77;
  }
}
