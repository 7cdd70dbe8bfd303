// teaser::Matcher::calculateKnnCorrespondences / ...Batch through the drop-in header.
//   knn_example FILE K MUTUAL   FILE: int32 n_src, int32 n_dst, then n_src x 33 and n_dst x 33 floats.  Prints
//                               "pairs N" and one "i j" line per pair (the test compares them with the Python call).
//   knn_example                 features from a fixed integer recurrence, quantised so that ties are everywhere:
//                               k = 1 mutual must equal calculateCorrespondences with the cross check, a pair in a
//                               batch (beside an empty one) must equal the pair alone, mutual must be a subset.
// Exit code: 0 ok, 77 no MI355X visible, 2 unreadable input, 1 wrong result.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "teaser/matcher.h"

static teaser::FPFHCloud synthetic(size_t n, uint32_t seed) {
  teaser::FPFHCloud f(n);
  uint32_t x = seed;
  for (size_t i = 0; i < n; ++i)
    for (int c = 0; c < 33; ++c) {
      x = x * 1664525u + 1013904223u;
      f[i].histogram[c] = (float)((x >> 24) % 3);
    }
  return f;
}

int main(int argc, char** argv) {
  try {
    teaser::Matcher matcher;
    if (argc >= 4) {
      std::FILE* fp = std::fopen(argv[1], "rb");
      int32_t n[2];
      if (!fp || std::fread(n, 4, 2, fp) != 2 || n[0] < 0 || n[1] < 0) return 2;
      teaser::FPFHCloud src((size_t)n[0]), dst((size_t)n[1]);
      const bool read = std::fread(src.data(), sizeof(teaser::FPFHSignature33), src.size(), fp) == src.size() &&
                        std::fread(dst.data(), sizeof(teaser::FPFHSignature33), dst.size(), fp) == dst.size();
      std::fclose(fp);
      if (!read) return 2;
      const auto pairs = matcher.calculateKnnCorrespondences(src, dst, std::atoi(argv[2]), std::atoi(argv[3]) != 0);
      std::printf("pairs %zu\n", pairs.size());
      for (const auto& p : pairs) std::printf("%d %d\n", p.first, p.second);
      return 0;
    }
    const teaser::FPFHCloud a = synthetic(300, 1), b = synthetic(170, 2);
    const teaser::PointCloud none;
    bool ok = matcher.calculateKnnCorrespondences(a, b, 1, true) ==
              matcher.calculateCorrespondences(none, none, a, b, false, true, false, 0);
    const auto mutual = matcher.calculateKnnCorrespondences(a, b, 3, true);
    const auto all = matcher.calculateKnnCorrespondences(a, b, 3, false);
    ok = ok && all.size() == 3 * a.size() && !mutual.empty() &&
         std::includes(all.begin(), all.end(), mutual.begin(), mutual.end());
    const auto batch = matcher.calculateKnnCorrespondencesBatch({a, teaser::FPFHCloud(), b}, {b, a, a}, 3, true);
    ok = ok && batch.size() == 3 && batch[0] == mutual && batch[1].empty() &&
         batch[2] == matcher.calculateKnnCorrespondences(b, a, 3, true);
    std::printf("k = 3: %zu mutual of %zu pairs  checks %d\n", mutual.size(), all.size(), (int)ok);
    return ok ? 0 : 1;
  } catch (const std::runtime_error& e) {
    std::printf("facade: %s\n", e.what());
    return 77;
  }
}
