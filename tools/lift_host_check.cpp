// The sampled families' host helpers (ls-spa_amd/csrc/host_perms.cpp: lift_orderings_why, lift_stage_rows,
// cv_count_folds; host code, no HIP call) under the host sanitisers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -I ls-spa_amd/csrc \
//       tools/lift_host_check.cpp ls-spa_amd/csrc/host_perms.cpp -o tools/bin/lift_host_check && tools/bin/lift_host_check
// Every buffer is a vector of exactly the size the helpers are promised, so a read or write past it is reported.  The
// maps: the GPU test's (p = 5, labels -1 0 0 1 2), one group of everything (d = 1) and all baseline but one column.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>

#include "players.h"

using namespace lsspa;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main() {
  const std::vector<std::vector<int32_t>> maps = {{-1, 0, 0, 1, 2}, {0, 0, 0, 0, 0}, {-1, -1, -1, 0, -1}, {0}, {2, 1, 0}};
  std::vector<int32_t> mark;
  char msg[240];
  for (const auto& labels : maps) {
    const int p = (int)labels.size(), g = 1 + *std::max_element(labels.begin(), labels.end());
    PlayerMap m;
    CHECK(player_map_build(labels.data(), p, g, m) == nullptr);
    for (int per = 1; per <= 2; ++per)
      for (int64_t B : {1, 6, 7}) {
        std::vector<int32_t> perms((size_t)(B * g)), rows;
        for (int64_t s = 0; s < B; ++s)      // rotations of 0 .. g-1
          for (int j = 0; j < g; ++j) perms[(size_t)(s * g + j)] = (int32_t)((j + s) % g);
        CHECK(!lift_orderings_why("e", "B", perms.data(), B, p, g, g, 2, mark, msg, sizeof msg));
        for (int64_t s0 = 0; s0 < B; s0 += 4) {      // two cuts, the last one ragged
          const int64_t ns = std::min<int64_t>(4, B - s0);
          const int32_t* src = lift_stage_rows(m, g, perms.data(), s0, ns, per, p, rows);
          CHECK(src == rows.data() && rows.size() >= (size_t)(ns * per * p));
          std::vector<int32_t> staged(src, src + ns * per * p);      // every row a permutation of the columns, baseline first
          CHECK(!lift_orderings_why("e", "B", staged.data(), ns * per, p, 0, p, 1, mark, msg, sizeof msg));
          for (int64_t r = 0; r < ns * per; ++r)
            CHECK(std::equal(m.base.begin(), m.base.end(), staged.begin() + r * p));
        }
        std::vector<int32_t> own((size_t)(B * p));      // without a map: the caller's rows
        CHECK(lift_stage_rows(m, 0, own.data(), 1, B - 1, per, p, rows) == own.data() + p);
        perms.back() = g;      // out of range
        CHECK(lift_orderings_why("e", "B", perms.data(), B, p, g, g, 2, mark, msg, sizeof msg) == msg);
        CHECK(std::strstr(msg, "e: a row of perms is not a permutation of 0 .. g-1 (a player map is set"));
      }
  }
  CHECK(lift_orderings_why("e", "B", nullptr, 1, 5, 0, 5, 1, mark, msg, sizeof msg) &&
        !std::strcmp(msg, "e: perms is NULL, B < 1 or B p >= 2^31"));
  std::vector<int32_t> one(5);
  std::iota(one.begin(), one.end(), 0);
  CHECK(lift_orderings_why("e", "n", one.data(), 0, 5, 0, 5, 2, mark, msg, sizeof msg) &&
        !std::strcmp(msg, "e: perms is NULL, n < 1 or 2 n p >= 2^31"));
  CHECK(lift_orderings_why("e", "n", one.data(), (int64_t)INT32_MAX / 10 + 1, 5, 0, 5, 2, mark, msg, sizeof msg));
  for (int K : {2, 3, 32}) {      // fold labels: 24 rows (K = 32: more rows), a label out of range, an empty fold
    const int64_t n = K == 32 ? 64 : 24;
    std::vector<int32_t> ids((size_t)n), nf((size_t)K, -1);
    for (int64_t i = 0; i < n; ++i) ids[(size_t)i] = (int32_t)(i % K);
    CHECK(!cv_count_folds(ids.data(), n, K, nf.data(), msg, sizeof msg));
    CHECK(std::accumulate(nf.begin(), nf.end(), (int64_t)0) == n && nf[0] >= nf[(size_t)K - 1] && nf[(size_t)K - 1] >= 1);
    ids[3] = K;
    CHECK(cv_count_folds(ids.data(), n, K, nf.data(), msg, sizeof msg) == msg && std::strstr(msg, "fold_ids[3] = "));
    ids[3] = -1;
    CHECK(cv_count_folds(ids.data(), n, K, nf.data(), msg, sizeof msg) == msg);
    for (auto& f : ids) f = f == K - 1 ? 0 : f;
    ids[3] = 0;
    CHECK(cv_count_folds(ids.data(), n, K, nf.data(), msg, sizeof msg) == msg && std::strstr(msg, "is empty"));
  }
  std::printf("lift host helpers: ok\n");
  return 0;
}
