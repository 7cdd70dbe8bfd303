// teaser::Matcher::tupleTestBatch and the k-NN calls' tuple arguments through the drop-in header.  No input file:
// the scene comes from a fixed integer recurrence -- 400 points, a rotation of 0.7 rad about z, 200 consistent
// correspondences and about 120 random ones -- and every batched result is compared with teaser_hip_tuple_test (the
// host routine, the specification) called in this program for the same problem and seed.
// Exit code: 0 ok, 77 no MI355X visible, 1 wrong result.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "teaser/matcher.h"

using Pairs = std::vector<std::pair<int, int>>;

static uint32_t g_state = 12345u;
static uint32_t next_u32() {
  g_state = g_state * 1664525u + 1013904223u;
  return g_state >> 8;
}

static teaser::PointCloud cloud(size_t n) {
  teaser::PointCloud c;
  for (size_t i = 0; i < n; ++i) {
    const float x = (float)next_u32() / 16777216.0f, y = (float)next_u32() / 16777216.0f,
                z = (float)next_u32() / 16777216.0f;
    c.push_back({x, y, z});
  }
  return c;
}

static teaser::FPFHCloud features(size_t n) {
  teaser::FPFHCloud f(n);
  for (size_t i = 0; i < n; ++i)
    for (int c = 0; c < 33; ++c) f[i].histogram[c] = (float)(next_u32() % 3);
  return f;
}

static Pairs host(const teaser::PointCloud& src, const teaser::PointCloud& dst, Pairs pairs, float scale,
                  uint64_t seed) {
  int64_t cnt = (int64_t)pairs.size();
  const int32_t rc = teaser_hip_tuple_test(nullptr, reinterpret_cast<const float*>(src.data()), (int32_t)src.size(),
                                           reinterpret_cast<const float*>(dst.data()), (int32_t)dst.size(), scale, seed,
                                           reinterpret_cast<int32_t*>(pairs.data()), &cnt);
  if (rc != TEASER_HIP_OK) throw std::logic_error("teaser_hip_tuple_test refused the scene");
  pairs.resize((size_t)cnt);
  return pairs;
}

int main() {
  try {
    const teaser::PointCloud src = cloud(400);
    teaser::PointCloud dst;
    const float c = std::cos(0.7f), s = std::sin(0.7f);
    for (const auto& p : src) dst.push_back({c * p.x - s * p.y + 0.3f, s * p.x + c * p.y - 0.2f, p.z + 0.1f});
    Pairs pairs;
    for (int i = 0; i < 200; ++i) pairs.emplace_back(i, i);
    for (int i = 200; i < 320; ++i) {
      const int j = (int)(next_u32() % 400u);
      if (j != i) pairs.emplace_back(i, j);
    }
    Pairs reversed(pairs.rbegin(), pairs.rend());
    reversed.insert(reversed.end(), pairs.begin(), pairs.begin() + 10);  // unsorted, with repeats

    teaser::Matcher matcher;
    const auto out = matcher.tupleTestBatch({src, src, src}, {dst, dst, dst}, {pairs, reversed, Pairs()}, 0.95f, 11);
    const Pairs want = host(src, dst, pairs, 0.95f, 11);
    int n_check = 0, failed = 0;
    bool ok = true;
    const auto check = [&](bool c) {
      if (!c) failed |= 1 << n_check;
      ++n_check;
      ok = ok && c;
    };
    check(out.size() == 3 && out[0] == want && out[1] == host(src, dst, reversed, 0.95f, 11) && out[2].empty());
    check(want.size() >= 200 && want.size() < pairs.size() &&
          std::includes(want.begin(), want.end(), pairs.begin(), pairs.begin() + 200));
    check(matcher.tupleTestBatch({src}, {dst}, {pairs}, 0.95f, 12)[0] == host(src, dst, pairs, 0.95f, 12));
    check(matcher.tupleTestBatch({src}, {dst}, {reversed}, 0.0f, 11)[0] == reversed);  // scale 0: untouched

    // the k-NN calls with a tuple scale = the calls without it, then the host routine; points for 300 / 170 rows
    const teaser::FPFHCloud fa = features(300), fb = features(170);
    const teaser::PointCloud pa = cloud(300), pb = cloud(170);
    const auto knn = matcher.calculateKnnCorrespondencesBatch({fa, fb}, {fb, fa}, 3, false);
    const auto knn_tuple = matcher.calculateKnnCorrespondencesBatch({fa, fb}, {fb, fa}, 3, false, 0.95f, 7, {pa, pb}, {pb, pa});
    check(knn.size() == 2 && knn[0].size() == 900 && knn_tuple.size() == 2);
    check(knn_tuple[0] == host(pa, pb, knn[0], 0.95f, 7) && knn_tuple[1] == host(pb, pa, knn[1], 0.95f, 7));
    check(!knn_tuple[0].empty() && knn_tuple[0].size() < knn[0].size());
    check(matcher.calculateKnnCorrespondences(fa, fb, 3, false, 0.95f, 7, pa, pb) == knn_tuple[0]);
    check(matcher.calculateKnnCorrespondences(fa, fb, 3, false) == knn[0]);
    // calculateCorrespondencesBatch seeds its tuple test from the clock, like the reference: a sorted subset
    const auto plain = matcher.calculateCorrespondencesBatch({pa}, {pb}, {fa}, {fb}, true, true, false, 0);
    const auto clock = matcher.calculateCorrespondencesBatch({pa}, {pb}, {fa}, {fb}, true, true, true, 0.95f);
    check(std::is_sorted(clock[0].begin(), clock[0].end()) &&
          std::includes(plain[0].begin(), plain[0].end(), clock[0].begin(), clock[0].end()));
    std::printf("tuple test: %zu of %zu pairs, k-NN %zu of %zu  checks %d (failed mask 0x%x)\n", want.size(),
                pairs.size(), knn_tuple[0].size(), knn[0].size(), (int)ok, (unsigned)failed);
    return ok ? 0 : 1;
  } catch (const std::runtime_error& e) {
    std::printf("facade: %s\n", e.what());
    return 77;
  }
}
