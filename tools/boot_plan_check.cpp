// The bootstrap's block planner (ls-spa_amd/csrc/boot_plan.cpp: host code, no HIP call) under the host sanitisers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ls-spa_amd/csrc \
//       tools/boot_plan_check.cpp ls-spa_amd/csrc/boot_plan.cpp -o tools/bin/boot_plan_check && tools/bin/boot_plan_check
// Sweeps R, N, M, p and block over their edges (1, the 16-column block edges, the row limit 2^31 - 1, block requests
// beyond the memory bound) and checks what the callers rely on: at least one replicate a block, blocks that cover R,
// the memory bound wherever one replicate fits it, slices that cover the rows, enumeration launches within their bound.
// Then the same for the grouped planner (boot_groups_plan) up to p = 64, and both planners' refusals.  The interaction
// planners (boot_inter_plan, boot_groups_inter_plan) ride the same sweeps: the Gram side is the phi planner's, steps is
// the one-problem call's cut whatever R and block are, units * enum_reps * steps <= 2^20 (grouped: and the work bound),
// and block * rep_bytes + table_bytes <= BOOT_BLOCK_BYTES or block == 1.  The best-subset planner (boot_best_plan) too:
// boot_plan's Gram side and units, 16 bytes a table entry in rep_bytes, per within the kernel's size classes; and its
// grouped sibling (boot_groups_best_plan) on the grouped sweep: boot_groups_plan's Gram side, units and per, 16 bytes an
// entry, units * enum_reps <= 2^20 workgroups, and the work bound unless one step of one replicate is already more.
// The sampled bootstrap's planner (boot_lift_plan) up to p = 127: boot_plan's slices, the Gram and lift kernel forms at
// their column-block edges, lift launches within their grid and raw-lift bounds, a sample cut that is not R's or the block's.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

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
            CHECK(P.table_bytes == 0);
            BootPlan I;
            CHECK(boot_inter_plan(R, N, M, p, block, I) == nullptr);
            CHECK(I.cb == P.cb && I.ldz == P.ldz && I.pairs == P.pairs && I.rpw == P.rpw);
            for (int s = 0; s < 2; ++s) CHECK(I.rps[s] == P.rps[s] && I.slices[s] == P.slices[s]);
            CHECK(I.units == P.units && I.per == P.per);
            CHECK(I.steps == (I.per < BOOT_SUBSETS_PER_LAUNCH / I.units ? I.per : BOOT_SUBSETS_PER_LAUNCH / I.units));
            CHECK(I.steps >= 1 && I.steps <= I.per);
            CHECK(I.block >= 1 && I.block <= R && I.block <= BOOT_MAX_BLOCK && (block == 0 || I.block <= block));
            CHECK(I.n_blocks >= 1 && (I.n_blocks - 1) * I.block < R && I.n_blocks * I.block >= R);
            CHECK(I.enum_reps >= 1 && I.enum_reps <= I.block && I.enum_reps <= 65535);
            CHECK(I.units * (uint64_t)I.enum_reps * I.steps <= BOOT_SUBSETS_PER_LAUNCH);
            CHECK(I.table_bytes == I.enum_reps * (int64_t)I.units * boot_inter_cols(p) * 8);
            CHECK(I.block == 1 || I.block * I.rep_bytes + I.table_bytes <= BOOT_BLOCK_BYTES);
            CHECK(I.rep_bytes >= 8 * (N + M) + 8 * boot_inter_cols(p));
            BootPlan B;      // the best-subset run: boot_plan's Gram side and units, a table entry of 16 bytes
            CHECK(boot_best_plan(R, N, M, p, block, B) == nullptr);
            CHECK(B.cb == P.cb && B.ldz == P.ldz && B.pairs == P.pairs && B.rpw == P.rpw);
            for (int s = 0; s < 2; ++s) CHECK(B.rps[s] == P.rps[s] && B.slices[s] == P.slices[s]);
            CHECK(B.units == P.units && B.per == P.per && B.per <= BOOT_BEST_MAX_PER);
            CHECK(B.rep_bytes == P.rep_bytes + (int64_t)B.units * (p + 1) * 8);
            CHECK(B.block >= 1 && B.block <= R && B.block <= P.block && (block == 0 || B.block <= block));
            CHECK(B.n_blocks >= 1 && (B.n_blocks - 1) * B.block < R && B.n_blocks * B.block >= R);
            CHECK(B.block == 1 || B.block * B.rep_bytes <= BOOT_BLOCK_BYTES);
            CHECK(B.enum_reps >= 1 && B.enum_reps <= B.block && B.enum_reps <= 65535 && B.steps >= 1 && B.steps <= B.per);
            CHECK(B.units * (uint64_t)B.enum_reps * B.steps <= BOOT_SUBSETS_PER_LAUNCH && B.table_bytes == 0);
            ++n_ok;
          }
  // The grouped planner (boot_groups_plan): every p up to 64 with layouts of gh high groups, nb baseline and ql low
  // columns at their edges -- no high group, no low group, gh = 26 (the most that 64 columns hold beside six low
  // singletons), a baseline that leaves one column a group
  struct Lay { int g, gh, nb, ql; };
  const int64_t rows_test[] = {1, 513, (1ll << 31) - 1};
  for (int64_t R : reps)
    for (int64_t N : rows)
      for (int64_t M : rows_test)
        for (int p = 1; p <= 64; ++p)
          for (int64_t block : blocks) {
            const int six = p < 6 ? p : 6;
            const Lay lays[] = {{1, p > 6 ? 1 : 0, 0, p > 6 ? 0 : p},            // the columns as one group
                                {six, 0, p - six, six},                          // low singletons, the rest baseline
                                {p < 32 ? p : 32, (p < 32 ? p : 32) - six, 0, six},   // as many groups as fit
                                {p > 6 ? 2 : 1, p > 6 ? 1 : 0, p > 6 ? 1 : 0, p > 6 ? 3 : p}};
            for (const Lay& L : lays) {
              BootPlan P;
              CHECK(boot_groups_plan(R, N, M, p, L.g, L.gh, L.nb, L.ql, block, P) == nullptr);
              CHECK(P.cb == (p + 16) / 16 && P.cb <= 5 && P.ldz == 16 * P.cb && P.pairs == P.cb * (P.cb + 1) / 2);
              CHECK(P.rpw == (P.cb <= 2 ? 4 : P.cb == 3 ? 2 : 1) && P.rpw * P.pairs * 4 <= 60);
              CHECK(P.block >= 1 && P.block <= R && P.block <= BOOT_MAX_BLOCK && (block == 0 || P.block <= block));
              CHECK(P.n_blocks >= 1 && (P.n_blocks - 1) * P.block < R && P.n_blocks * P.block >= R);
              CHECK(P.block == 1 || P.block * P.rep_bytes <= BOOT_BLOCK_BYTES);
              BootPlan Q;      // the slices are the ungrouped planner's for the same rows
              CHECK(boot_plan(R, N, M, 1, block, Q) == nullptr);
              for (int s = 0; s < 2; ++s) CHECK(P.rps[s] == Q.rps[s] && P.slices[s] == Q.slices[s]);
              CHECK(P.enum_reps >= 1 && P.enum_reps <= P.block &&
                    P.units * (uint64_t)P.enum_reps <= BOOT_SUBSETS_PER_LAUNCH);
              CHECK(P.units * P.per == (1ull << L.gh) && P.units <= BOOT_UNITS && P.steps >= 1 && P.steps <= P.per);
              // the cut of `per` into launches is the layout's alone: not R's, the block's or the rows'
              CHECK(boot_groups_plan(1, 1, 1, p, L.g, L.gh, L.nb, L.ql, 0, Q) == nullptr && Q.steps == P.steps &&
                    Q.units == P.units && Q.per == P.per);
              CHECK(P.table_bytes == 0);
              BootPlan I;
              CHECK(boot_groups_inter_plan(R, N, M, p, L.g, L.gh, L.nb, L.ql, block, I) == nullptr);
              CHECK(I.cb == P.cb && I.ldz == P.ldz && I.pairs == P.pairs && I.rpw == P.rpw);
              for (int s = 0; s < 2; ++s) CHECK(I.rps[s] == P.rps[s] && I.slices[s] == P.slices[s]);
              CHECK(I.units == P.units && I.per == P.per && I.steps == P.steps);
              CHECK(I.block >= 1 && I.block <= R && I.block <= BOOT_MAX_BLOCK && (block == 0 || I.block <= block));
              CHECK(I.n_blocks >= 1 && (I.n_blocks - 1) * I.block < R && I.n_blocks * I.block >= R);
              CHECK(I.enum_reps >= 1 && I.enum_reps <= I.block && I.enum_reps <= 65535);
              CHECK(I.units * (uint64_t)I.enum_reps * I.steps <= BOOT_SUBSETS_PER_LAUNCH);
              const uint64_t mrows = (uint64_t)(L.nb + L.ql + 1) + (uint64_t)(p - L.nb - L.ql + 1) / 2;
              CHECK(I.enum_reps == 1 ||
                    I.units * (uint64_t)I.enum_reps * I.steps * mrows * mrows <= BOOT_GROUPS_WORK_PER_LAUNCH);
              CHECK(I.table_bytes == I.enum_reps * (int64_t)I.units * boot_inter_cols(L.g) * 8);
              CHECK(I.block == 1 || I.block * I.rep_bytes + I.table_bytes <= BOOT_BLOCK_BYTES);
              BootPlan B;      // the best-subset run over groups: that Gram side, units and per, a table entry of 16 bytes
              CHECK(boot_groups_best_plan(R, N, M, p, L.g, L.gh, L.nb, L.ql, block, B) == nullptr);
              CHECK(B.cb == P.cb && B.ldz == P.ldz && B.pairs == P.pairs && B.rpw == P.rpw);
              for (int s = 0; s < 2; ++s) CHECK(B.rps[s] == P.rps[s] && B.slices[s] == P.slices[s]);
              CHECK(B.units == P.units && B.per == P.per && B.per <= BOOT_GROUPS_BEST_MAX_PER);
              CHECK(B.rep_bytes == P.rep_bytes + (int64_t)B.units * (L.g + 1) * 8);
              CHECK(B.block >= 1 && B.block <= R && B.block <= P.block && (block == 0 || B.block <= block));
              CHECK(B.n_blocks >= 1 && (B.n_blocks - 1) * B.block < R && B.n_blocks * B.block >= R);
              CHECK(B.block == 1 || B.block * B.rep_bytes <= BOOT_BLOCK_BYTES);
              CHECK(B.enum_reps >= 1 && B.enum_reps <= B.block && B.enum_reps <= 65535 && B.steps >= 1 && B.steps <= B.per);
              CHECK(B.units * (uint64_t)B.enum_reps <= BOOT_SUBSETS_PER_LAUNCH && B.table_bytes == 0);
              CHECK((B.enum_reps == 1 && B.steps == 1) ||
                    B.units * (uint64_t)B.enum_reps * B.steps * mrows * mrows <= BOOT_GROUPS_WORK_PER_LAUNCH);
              ++n_ok;
            }
          }
  {
    int64_t R = 1, N = 1, M = 1, block = 0;
    int p = 8;
    BootPlan P;
    CHECK(boot_groups_plan(1, 1, 1, 65, 1, 1, 0, 0, 0, P) && boot_groups_plan(1, 1, 1, 0, 1, 1, 0, 0, 0, P));
    CHECK(boot_groups_plan(1, 1, 1, 40, 33, 27, 0, 6, 0, P) && boot_groups_plan(1, 1, 1, 8, 0, 0, 0, 0, 0, P));
    CHECK(boot_groups_plan(1, 1, 1, 8, 2, 3, 0, 0, 0, P) && boot_groups_plan(1, 1, 1, 8, 2, 1, 0, 7, 0, P));
    CHECK(boot_groups_plan(1, 1, 1, 8, 8, 1, 0, 6, 0, P) && boot_groups_plan(1, 1, 1, 8, 2, 1, 8, 1, 0, P));
    CHECK(boot_groups_plan(0, 1, 1, 8, 2, 1, 0, 1, 0, P) && boot_groups_plan(1, 1, 1ll << 31, 8, 2, 1, 0, 1, 0, P));
    CHECK(boot_groups_plan(1, 1, 1, 8, 2, 1, 0, 1, -1, P) && !boot_groups_plan(1, 1, 1, 8, 2, 1, 0, 1, 0, P));
    CHECK(boot_groups_inter_plan(1, 1, 1, 65, 1, 1, 0, 0, 0, P) && boot_groups_inter_plan(1, 1, 1, 40, 33, 27, 0, 6, 0, P));
    CHECK(boot_groups_inter_plan(0, 1, 1, 8, 2, 1, 0, 1, 0, P) && boot_groups_inter_plan(1, 1, 1, 8, 2, 1, 0, 1, -1, P));
    CHECK(!boot_groups_inter_plan(1, 1, 1, 8, 2, 1, 0, 1, 0, P));
    CHECK(boot_groups_best_plan(1, 1, 1, 65, 1, 1, 0, 0, 0, P) && boot_groups_best_plan(1, 1, 1, 40, 33, 27, 0, 6, 0, P));
    CHECK(boot_groups_best_plan(0, 1, 1, 8, 2, 1, 0, 1, 0, P) && boot_groups_best_plan(1, 1, 1, 8, 2, 1, 0, 1, -1, P));
    CHECK(boot_groups_best_plan(1, 1, 1, 8, 2, 3, 0, 0, 0, P) && !boot_groups_best_plan(1, 1, 1, 8, 2, 1, 0, 1, 0, P));
    CHECK(boot_inter_plan(0, 1, 1, 1, 0, P) && boot_inter_plan(1, 0, 1, 1, 0, P) && boot_inter_plan(1, 1, 1ll << 31, 1, 0, P));
    CHECK(boot_inter_plan(1, 1, 1, 33, 0, P) && boot_inter_plan(1, 1, 1, 0, 0, P) && boot_inter_plan(1, 1, 1, 1, -1, P));
    CHECK(boot_best_plan(0, 1, 1, 1, 0, P) && boot_best_plan(1, 0, 1, 1, 0, P) && boot_best_plan(1, 1, 1ll << 31, 1, 0, P));
    CHECK(boot_best_plan(1, 1, 1, 33, 0, P) && boot_best_plan(1, 1, 1, 0, 0, P) && boot_best_plan(1, 1, 1, 1, -1, P));
    // group layouts up to (g, p) = (32, 64): 26 high groups of one or two columns beside six low singletons
    for (int g = 7; g <= 32; ++g) {
      p = 64;
      R = 1000;
      N = M = 100000;
      for (int64_t blk : {0ll, 1ll, 3ll}) {
        block = blk;
        BootPlan I, Q;
        CHECK(boot_groups_inter_plan(R, N, M, p, g, g - 6, 0, 6, block, I) == nullptr);
        CHECK(boot_groups_plan(1, 1, 1, p, g, g - 6, 0, 6, 0, Q) == nullptr && Q.steps == I.steps && Q.units == I.units);
        CHECK(I.units * (uint64_t)I.enum_reps * I.steps <= BOOT_SUBSETS_PER_LAUNCH && I.enum_reps >= 1);
        CHECK(I.block == 1 || I.block * I.rep_bytes + I.table_bytes <= BOOT_BLOCK_BYTES);
        BootPlan B;
        CHECK(boot_groups_best_plan(R, N, M, p, g, g - 6, 0, 6, block, B) == nullptr && B.units == Q.units);
        CHECK(B.per <= BOOT_GROUPS_BEST_MAX_PER && B.steps >= 1 && B.steps <= B.per && B.enum_reps >= 1);
        CHECK(B.units * (uint64_t)B.enum_reps <= BOOT_SUBSETS_PER_LAUNCH);
        CHECK((B.enum_reps == 1 && B.steps == 1) ||
              B.units * (uint64_t)B.enum_reps * B.steps * 36 * 36 <= BOOT_GROUPS_WORK_PER_LAUNCH);   // rows: 7 + 59 / 2
        CHECK(B.block == 1 || B.block * B.rep_bytes <= BOOT_BLOCK_BYTES);
        ++n_ok;
      }
    }
    // the table does not cut a block to a handful of replicates at large p
    R = 1000; N = M = 10000; block = 0; p = 32;
    CHECK(boot_inter_plan(R, N, M, p, block, P) == nullptr && P.enum_reps == 1 && P.block >= 100);
  }
  // The sampled bootstrap's planner (boot_lift_plan): every p up to 127, samples at the launch cut's edges, both pair
  // settings.  The Gram side is boot_plan's for the same rows; the sample cut is a function of n_samples and the pair
  // setting alone; a lift launch stays within its grid and raw-lift bounds whatever R and block are.
  {
    const int64_t rows_l[] = {1, 257, 100000, (1ll << 31) - 1};
    const int64_t samples[] = {1, 2, 127, 128, 129, 256, 257, 1024, 1ll << 30};
    for (int64_t R : reps)
      for (int64_t N : rows_l)
        for (int64_t M : rows_l)
          for (int p = 1; p <= BOOT_LIFT_MAX_P; ++p)
            for (int64_t block : blocks)
              for (int64_t ns : samples)
                for (int anti = 0; anti < 2; ++anti) {
                  const int d = p > 3 ? p / 3 : p;
                  BootLiftPlan L, L1;
                  CHECK(boot_lift_plan(R, N, M, p, anti ? d : p, ns, anti, block, L) == nullptr);
                  CHECK(L.cb == (p + 16) / 16 && L.cb <= 8 && L.ldz == 16 * L.cb && L.pairs == L.cb * (L.cb + 1) / 2);
                  CHECK(L.gram_form == (L.cb >= 6) && L.lift_form == (L.cb == 8));
                  CHECK(L.rpw == (L.cb <= 2 ? 4 : L.cb == 3 ? 2 : 1));
                  BootPlan Q;
                  CHECK(boot_plan(R, N, M, 1, block, Q) == nullptr);
                  for (int s = 0; s < 2; ++s) CHECK(L.rps[s] == Q.rps[s] && L.slices[s] == Q.slices[s]);
                  CHECK(L.block >= 1 && L.block <= R && L.block <= BOOT_MAX_BLOCK && (block == 0 || L.block <= block));
                  CHECK(L.n_blocks >= 1 && (L.n_blocks - 1) * L.block < R && L.n_blocks * L.block >= R);
                  CHECK(L.block == 1 || L.block * L.rep_bytes <= BOOT_BLOCK_BYTES);
                  const int64_t per = anti ? 2 : 1;
                  CHECK(L.samples_per_launch >= 1 && L.samples_per_launch <= ns && L.ord_per_launch == per * L.samples_per_launch);
                  CHECK(L.ord_per_launch <= BOOT_LIFT_ORD && L.sample_cuts * L.samples_per_launch >= ns &&
                        (L.sample_cuts - 1) * L.samples_per_launch < ns);
                  CHECK(L.reps_per_launch >= 1 &&
                        L.ord_per_launch * L.reps_per_launch <= (L.lift_form ? BOOT_LIFT_GRID_LDS : BOOT_LIFT_GRID_REG));
                  CHECK(L.ord_per_launch * L.reps_per_launch * p * 8 <= BOOT_LIFT_RAW_BYTES && L.raw_bytes <= BOOT_LIFT_RAW_BYTES);
                  CHECK(L.launches == INT64_MAX || L.launches / L.sample_cuts >= L.n_blocks);   // (it saturates)
                  // the cut is not R's, the block's or the rows'
                  CHECK(boot_lift_plan(1, 1, 1, p, anti ? d : p, ns, anti, 0, L1) == nullptr);
                  CHECK(L1.samples_per_launch == L.samples_per_launch && L1.reps_per_launch == L.reps_per_launch &&
                        L1.sample_cuts == L.sample_cuts);
                  ++n_ok;
                }
    BootLiftPlan L;
    if (!(boot_lift_plan(1, 1, 1, 128, 1, 1, 0, 0, L) && boot_lift_plan(1, 1, 1, 0, 1, 1, 0, 0, L) &&
          boot_lift_plan(1, 1, 1, 4, 5, 1, 0, 0, L) && boot_lift_plan(1, 1, 1, 4, 0, 1, 0, 0, L) &&
          boot_lift_plan(1, 1, 1, 4, 4, 0, 0, 0, L) && boot_lift_plan(0, 1, 1, 4, 4, 1, 0, 0, L) &&
          boot_lift_plan(1, 1, 1ll << 31, 4, 4, 1, 0, 0, L) && boot_lift_plan(1, 1, 1, 4, 4, 1, 0, -1, L))) {
      std::fprintf(stderr, "FAILED: boot_lift_plan accepted a bad argument\n");
      return 1;
    }
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
