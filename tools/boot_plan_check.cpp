// The bootstrap's block planner (ls-spa_amd/csrc/boot_plan.cpp: host code, no HIP call) under the host sanitisers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ls-spa_amd/csrc \
//       tools/boot_plan_check.cpp ls-spa_amd/csrc/boot_plan.cpp -o tools/bin/boot_plan_check && tools/bin/boot_plan_check
// Sweeps R, N, M, p and block over their edges (1, the 16-column block edges, the row limit 2^31 - 1, block requests
// beyond the memory bound) and checks what the callers rely on: at least one replicate a block, blocks that cover R,
// the memory bound wherever one replicate fits it, slices that cover the rows, enumeration launches within their bound.
#include <cstdio>
#include <cstdlib>

#include "boot_plan.h"

using namespace lsspa;

#define CHECK(c)                                                                                    \
  do {                                                                                              \
    if (!(c)) {                                                                                     \
      std::fprintf(stderr, "FAILED %s (R %lld N %lld M %lld p %d block %lld)\n", #c, (long long)R, \
                   (long long)N, (long long)M, p, (long long)block);                                \
      return 1;                                                                                     \
    }                                                                                               \
  } while (0)

int main() {
  const int64_t rows[] = {1, 3, 4, 5, 255, 256, 257, 512, 513, 100000, (1ll << 31) - 1};
  const int64_t reps[] = {1, 2, 15, 16, 17, 1000, 1ll << 40};
  const int64_t blocks[] = {0, 1, 3, 16, 1024, 1025, 1ll << 50};
  long n_ok = 0;
  for (int64_t R : reps)
    for (int64_t N : rows)
      for (int64_t M : rows)
        for (int p = 1; p <= 32; ++p)
          for (int64_t block : blocks) {
            BootPlan P;
            CHECK(boot_plan(R, N, M, p, block, P) == nullptr);
            CHECK(P.cb == (p + 16) / 16 && P.ldz == 16 * P.cb && P.pairs == P.cb * (P.cb + 1) / 2);
            CHECK(P.block >= 1 && P.block <= R && P.block <= BOOT_MAX_BLOCK && (block == 0 || P.block <= block));
            CHECK(P.n_blocks >= 1 && (P.n_blocks - 1) * P.block < R && P.n_blocks * P.block >= R);
            CHECK(P.block == 1 || P.block * P.rep_bytes <= BOOT_BLOCK_BYTES);
            const int64_t n[2] = {N, M};
            for (int s = 0; s < 2; ++s) {
              CHECK(P.rps[s] >= BOOT_MIN_SLICE_ROWS && P.rps[s] % 4 == 0 && P.slices[s] >= 1);
              CHECK(P.slices[s] <= BOOT_MAX_SLICES && (int64_t)P.slices[s] * P.rps[s] >= n[s]);
              CHECK((int64_t)(P.slices[s] - 1) * P.rps[s] < n[s]);
            }
            CHECK(P.enum_reps >= 1 && P.enum_reps <= P.block && P.units * (uint64_t)P.enum_reps <= BOOT_SUBSETS_PER_LAUNCH);
            CHECK(P.units * P.per == (1ull << (p < BOOT_LOW ? 0 : p - BOOT_LOW)) && P.steps >= 1 && P.steps <= P.per);
            ++n_ok;
          }
  BootPlan P;
  const bool refused = boot_plan(0, 1, 1, 1, 0, P) && boot_plan(1, 0, 1, 1, 0, P) && boot_plan(1, 1, 1ll << 31, 1, 0, P) &&
                       boot_plan(1, 1, 1, 33, 0, P) && boot_plan(1, 1, 1, 0, 0, P) && boot_plan(1, 1, 1, 1, -1, P);
  if (!refused) {
    std::fprintf(stderr, "FAILED: a bad argument was accepted\n");
    return 1;
  }
  std::printf("boot_plan: %ld plans checked\n", n_ok);
  return 0;
}
