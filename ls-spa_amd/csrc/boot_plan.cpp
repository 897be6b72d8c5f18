// How a bootstrap run is cut (lsspa_boot_run): row slices of the weighted Gram pass, replicates per block, replicates and
// steps per enumeration launch.  Host code only, no HIP call: lsspa_debug_boot_plan and a stand-alone sanitiser build
// (tools/boot_plan_check.cpp) exercise it without a GPU.
#include "boot_plan.h"

#include <algorithm>

namespace lsspa {

namespace {

// what the rows and the columns decide: the column blocks of Z, replicates per wave and the row slices of both sides
void plan_gram(int64_t N, int64_t M, int c, BootPlan& P) {
  P.cb = (c + 15) / 16;
  P.ldz = 16 * P.cb;
  P.pairs = P.cb * (P.cb + 1) / 2;
  // accumulators a wave holds: rpw * pairs * 4 doubles a lane (<= 96 registers up to cb = 3; 80 and 120 at cb = 4, 5)
  P.rpw = P.cb <= 2 ? 4 : P.cb == 3 ? 2 : 1;
  const int64_t rows[2] = {N, M};
  for (int s = 0; s < 2; ++s) {
    // a slice: at least BOOT_MIN_SLICE_ROWS rows, at most BOOT_MAX_SLICES of them -- a function of the rows alone, so
    // that a replicate's sums do not depend on how many replicates share its block
    int64_t rps = (rows[s] + BOOT_MAX_SLICES - 1) / BOOT_MAX_SLICES;
    rps = std::max<int64_t>(BOOT_MIN_SLICE_ROWS, (rps + 3) / 4 * 4);
    P.rps[s] = rps;
    P.slices[s] = (int)((rows[s] + rps - 1) / rps);
  }
}

// per replicate: weights of both sides (8 bytes a row: fp64 weights; counts take half), the Gram partials of both
// sides, the enumeration's partial table [units][players + 1], and the small per-replicate matrices (S, G, H, ...
// < 8 c^2 doubles); then the replicates of a block and the blocks
// entry: the bytes of one entry of that table (8: a sum; 16: the best run's value, mask and found flag)
void plan_blocks(int64_t R, int64_t N, int64_t M, int c, int players, int64_t block, BootPlan& P, int entry = 8) {
  P.rep_bytes = 8 * (N + M) + (int64_t)(P.slices[0] + P.slices[1]) * P.pairs * 256 * 8 +
                (int64_t)P.units * (players + 1) * entry + 8ll * c * c * 8;
  int64_t most = std::max<int64_t>(1, std::min<int64_t>(BOOT_MAX_BLOCK, BOOT_BLOCK_BYTES / P.rep_bytes));
  P.block = std::min<int64_t>(R, block > 0 ? std::min(block, most) : most);
  P.n_blocks = (R + P.block - 1) / P.block;
}

// The interaction planners' blocks: the partial table [enum_reps][units][cols] is one launch's and stands beside the
// block; launch_reps: the replicates a launch of P.steps steps may take by its launch bounds.  Needs units, steps.
void plan_inter_blocks(int64_t R, int64_t N, int64_t M, int c, int cols, uint64_t launch_reps, int64_t block,
                       BootPlan& P) {
  const int64_t rep_table = (int64_t)P.units * cols * 8;
  const int64_t most_reps = std::max<int64_t>(
      1, std::min<int64_t>({BOOT_MAX_BLOCK, (int64_t)std::min<uint64_t>(launch_reps, 1ull << 30),
                            BOOT_INTER_TABLE_BYTES / rep_table}));
  P.rep_bytes = 8 * (N + M) + (int64_t)(P.slices[0] + P.slices[1]) * P.pairs * 256 * 8 + (int64_t)cols * 8 +
                8ll * c * c * 8;
  const int64_t left = BOOT_BLOCK_BYTES - most_reps * rep_table;
  int64_t most = std::max<int64_t>(1, std::min<int64_t>(BOOT_MAX_BLOCK, left / P.rep_bytes));
  P.block = std::min<int64_t>(R, block > 0 ? std::min(block, most) : most);
  P.n_blocks = (R + P.block - 1) / P.block;
  P.enum_reps = std::min<int64_t>(P.block, most_reps);
  P.table_bytes = P.enum_reps * rep_table;
}

const char* plan_sizes(int64_t R, int64_t N, int64_t M, int64_t block) {
  if (R < 1) return "R must be at least 1";
  if (N < 1 || M < 1 || N >= (1ll << 31) || M >= (1ll << 31)) return "N and M must be 1 .. 2^31 - 1";
  if (block < 0) return "block must be >= 0";
  return nullptr;
}

}  // namespace

const char* boot_plan(int64_t R, int64_t N, int64_t M, int p, int64_t block, BootPlan& P) {
  P = BootPlan{};
  if (p < 1 || p > BOOT_MAX_P) return "p must be 1 .. 32";
  if (const char* why = plan_sizes(R, N, M, block)) return why;
  const int c = p + 1;
  plan_gram(N, M, c, P);
  const int q = p < BOOT_LOW ? p : BOOT_LOW;
  const uint64_t n_high = 1ull << (p - q);
  P.units = std::min<uint64_t>(n_high, BOOT_UNITS);
  P.per = n_high / P.units;
  plan_blocks(R, N, M, c, p, block, P);
  P.enum_reps = std::max<int64_t>(1, std::min<int64_t>(P.block, (int64_t)(BOOT_SUBSETS_PER_LAUNCH / P.units)));
  P.steps = std::max<uint64_t>(1, BOOT_SUBSETS_PER_LAUNCH / (P.units * (uint64_t)P.enum_reps));
  P.steps = std::min<uint64_t>(P.steps, P.per);
  return nullptr;
}

const char* boot_best_plan(int64_t R, int64_t N, int64_t M, int p, int64_t block, BootPlan& P) {
  P = BootPlan{};
  if (p < 1 || p > BOOT_MAX_P) return "p must be 1 .. 32";
  if (const char* why = plan_sizes(R, N, M, block)) return why;
  const int c = p + 1;
  plan_gram(N, M, c, P);
  const int q = p < BOOT_LOW ? p : BOOT_LOW;
  const uint64_t n_high = 1ull << (p - q);
  P.units = std::min<uint64_t>(n_high, BOOT_UNITS);
  P.per = n_high / P.units;
  if (P.per > BOOT_BEST_MAX_PER) return "more high subsets per unit than the best kernel's size classes hold";
  plan_blocks(R, N, M, c, p, block, P, 16);
  // The winner of a total order does not depend on the cut, so the cut is chosen for speed: a unit's steps first, as the
  // one-problem call cuts them (a workgroup loads its replicate's H and merges into its row once per launch), then as
  // many replicates as the launch has left
  P.steps = std::min<uint64_t>(P.per, std::max<uint64_t>(1, BOOT_SUBSETS_PER_LAUNCH / P.units));
  P.enum_reps = std::max<int64_t>(
      1, std::min<int64_t>(P.block, (int64_t)(BOOT_SUBSETS_PER_LAUNCH / (P.units * P.steps))));
  return nullptr;
}

const char* boot_groups_plan(int64_t R, int64_t N, int64_t M, int p, int g, int gh, int nb, int ql, int64_t block,
                             BootPlan& P) {
  P = BootPlan{};
  if (p < 1 || p > BOOT_GROUPS_MAX_P) return "p must be 1 .. 64";
  if (g < 1 || g > BOOT_GROUPS_MAX_G) return "g must be 1 .. 32";
  if (gh < 0 || gh > g || g - gh > BOOT_LOW || nb < 0 || ql < g - gh || ql > BOOT_LOW || nb + ql + gh > p || g > p)
    return "gh, nb, ql are not those of a layout of g groups over p columns";
  if (const char* why = plan_sizes(R, N, M, block)) return why;
  const int c = p + 1;
  plan_gram(N, M, c, P);
  const uint64_t n_high = 1ull << gh;
  P.units = std::min<uint64_t>(n_high, BOOT_UNITS);
  P.per = n_high / P.units;
  plan_blocks(R, N, M, c, g, block, P);
  // a launch: the work bound of the one-problem grouped enumeration (a high subset counts as the square of its matrix's
  // rows: baseline and low columns always, the high columns half of the time), and at most 2^20 workgroups.  A unit's
  // row of the partial table is the sum of its launches' sums, so how `per` is cut into launches shows in the bits:
  // `steps` is a function of the layout alone -- the one-problem call's own cut -- and never of R, the block or the
  // replicates a launch takes; those fill what a launch of `steps` steps leaves of the bound.
  const uint64_t rows = (uint64_t)(nb + ql + 1) + (uint64_t)(p - nb - ql + 1) / 2;
  const uint64_t per_launch = std::max<uint64_t>(1, BOOT_GROUPS_WORK_PER_LAUNCH / (rows * rows));
  P.steps = std::min<uint64_t>(P.per, std::max<uint64_t>(1, per_launch / P.units));
  const uint64_t groups = std::min<uint64_t>(BOOT_SUBSETS_PER_LAUNCH, per_launch) / (P.units * P.steps);
  P.enum_reps = std::max<int64_t>(1, std::min<int64_t>(P.block, (int64_t)groups));
  return nullptr;
}

const char* boot_groups_best_plan(int64_t R, int64_t N, int64_t M, int p, int g, int gh, int nb, int ql, int64_t block,
                                  BootPlan& P) {
  BootPlan Q;      // arguments, Gram side, units and per: the phi planner's
  if (const char* why = boot_groups_plan(R, N, M, p, g, gh, nb, ql, block, Q)) {
    P = BootPlan{};
    return why;
  }
  P = Q;
  // units = min(2^gh, BOOT_UNITS) and gh < g <= 32 or gh = g = 32 (which no layout of <= 64 columns has, and which
  // launch_groups_best refuses): the kernel's size classes hold every per a layout can give
  static_assert(((1ull << (BOOT_GROUPS_MAX_G - 1)) / BOOT_UNITS) <= BOOT_GROUPS_BEST_MAX_PER,
                "groups_best_kernel holds the size classes of the largest per: 31 high groups over BOOT_UNITS units");
  if (P.per > BOOT_GROUPS_BEST_MAX_PER) return "more high subsets per unit than the best kernel's size classes hold";
  plan_blocks(R, N, M, p + 1, g, block, P, 16);
  // The winner of a total order does not depend on the cut, so the cut is chosen for speed: a unit's steps first, as the
  // one-problem call cuts them (a workgroup loads its replicate's h and merges into its row once per launch), then as
  // many replicates as the work bound and the 2^20 workgroups leave such a launch
  const uint64_t rows = (uint64_t)(nb + ql + 1) + (uint64_t)(p - nb - ql + 1) / 2;
  const uint64_t per_launch = std::max<uint64_t>(1, BOOT_GROUPS_WORK_PER_LAUNCH / (rows * rows));
  P.steps = std::min<uint64_t>(P.per, std::max<uint64_t>(1, per_launch / P.units));
  const uint64_t reps = std::min<uint64_t>(BOOT_SUBSETS_PER_LAUNCH / P.units, per_launch / (P.units * P.steps));
  P.enum_reps = std::max<int64_t>(1, std::min<int64_t>(P.block, (int64_t)reps));
  return nullptr;
}

const char* boot_inter_plan(int64_t R, int64_t N, int64_t M, int p, int64_t block, BootPlan& P) {
  P = BootPlan{};
  if (p < 1 || p > BOOT_MAX_P) return "p must be 1 .. 32";
  if (const char* why = plan_sizes(R, N, M, block)) return why;
  const int c = p + 1;
  plan_gram(N, M, c, P);
  const int q = p < BOOT_LOW ? p : BOOT_LOW;
  const uint64_t n_high = 1ull << (p - q);
  P.units = std::min<uint64_t>(n_high, BOOT_UNITS);
  P.per = n_high / P.units;
  // the one-problem call's own cut: the players alone decide it
  P.steps = std::min<uint64_t>(P.per, std::max<uint64_t>(1, BOOT_SUBSETS_PER_LAUNCH / P.units));
  plan_inter_blocks(R, N, M, c, boot_inter_cols(p), BOOT_SUBSETS_PER_LAUNCH / (P.units * P.steps), block, P);
  return nullptr;
}

const char* boot_groups_inter_plan(int64_t R, int64_t N, int64_t M, int p, int g, int gh, int nb, int ql, int64_t block,
                                   BootPlan& P) {
  BootPlan Q;      // arguments, Gram side, units, per and steps: the phi planner's
  if (const char* why = boot_groups_plan(R, N, M, p, g, gh, nb, ql, block, Q)) {
    P = BootPlan{};
    return why;
  }
  P = Q;
  const uint64_t rows = (uint64_t)(nb + ql + 1) + (uint64_t)(p - nb - ql + 1) / 2;
  const uint64_t per_launch = std::max<uint64_t>(1, BOOT_GROUPS_WORK_PER_LAUNCH / (rows * rows));
  const uint64_t launch_reps = std::min<uint64_t>(BOOT_SUBSETS_PER_LAUNCH, per_launch) / (P.units * P.steps);
  plan_inter_blocks(R, N, M, p + 1, boot_inter_cols(g), launch_reps, block, P);
  return nullptr;
}

const char* boot_lift_plan(int64_t R, int64_t N, int64_t M, int p, int d, int64_t n_samples, int antithetical,
                           int64_t block, BootLiftPlan& P) {
  P = BootLiftPlan{};
  if (p < 1 || p > BOOT_LIFT_MAX_P) return "p must be 1 .. 127";
  if (d < 1 || d > p) return "d must be 1 .. p";
  if (n_samples < 1 || n_samples > (1ll << 30)) return "n_samples must be 1 .. 2^30";
  if (const char* why = plan_sizes(R, N, M, block)) return why;
  const int c = p + 1;
  BootPlan Q{};
  plan_gram(N, M, c, Q);
  P.cb = Q.cb;
  P.ldz = Q.ldz;
  P.pairs = Q.pairs;
  P.gram_form = Q.cb <= 5 ? 0 : 1;
  P.rpw = Q.rpw;                     // (1 from cb = 4 on)
  for (int s = 0; s < 2; ++s) {
    P.rps[s] = Q.rps[s];
    P.slices[s] = Q.slices[s];
  }
  // per replicate: weights of both sides, the Gram partials, S of both sides, the problem at the ordering kernels'
  // stride (G, H, g, h, inv_yy, the augmented diagonals), its running mean and M2 and its info word
  constexpr int64_t LD = BOOT_LIFT_LD;
  P.rep_bytes = 8 * (N + M) + (int64_t)(P.slices[0] + P.slices[1]) * P.pairs * 256 * 8 + 2ll * c * c * 8 +
                (2 * LD * LD + 2 * LD + 4) * 8 + 2ll * d * 8 + 8;
  const int64_t most = std::max<int64_t>(1, std::min<int64_t>(BOOT_MAX_BLOCK, BOOT_BLOCK_BYTES / P.rep_bytes));
  P.block = std::min<int64_t>(R, block > 0 ? std::min(block, most) : most);
  P.n_blocks = (R + P.block - 1) / P.block;
  const int64_t per = antithetical ? 2 : 1;
  P.lift_form = P.cb <= 7 ? 0 : 1;
  P.samples_per_launch = std::min<int64_t>(n_samples, BOOT_LIFT_ORD / per);
  P.ord_per_launch = P.samples_per_launch * per;
  P.sample_cuts = (n_samples + P.samples_per_launch - 1) / P.samples_per_launch;
  const int64_t grid = P.lift_form ? BOOT_LIFT_GRID_LDS : BOOT_LIFT_GRID_REG;
  P.reps_per_launch = std::max<int64_t>(
      1, std::min<int64_t>(grid / P.ord_per_launch, BOOT_LIFT_RAW_BYTES / (P.ord_per_launch * p * 8)));
  const int64_t full = R / P.block, rest = R - full * P.block;
  // (full <= R, a block has at most BOOT_MAX_BLOCK launch rows: the sum fits; the product saturates)
  const int64_t rep_launches = full * ((P.block + P.reps_per_launch - 1) / P.reps_per_launch) +
                               (rest + P.reps_per_launch - 1) / P.reps_per_launch;
  P.launches = rep_launches > INT64_MAX / P.sample_cuts ? INT64_MAX : rep_launches * P.sample_cuts;
  P.raw_bytes = P.ord_per_launch * std::min(P.reps_per_launch, P.block) * p * 8;
  return nullptr;
}

const char* perm_plan(int64_t R, int64_t N, int64_t M, int p, int64_t block, PermPlan& P) {
  P = PermPlan{};
  if (p < 1 || p > PERM_MAX_P) return "p must be 1 .. 64";
  if (const char* why = plan_sizes(R, N, M, block)) return why;
  P.cb = (p + 15) / 16;
  P.ldx = 16 * P.cb;
  const int64_t rows[2] = {N, M};
  for (int s = 0; s < 2; ++s) {
    int64_t rps = (rows[s] + PERM_MAX_SLICES - 1) / PERM_MAX_SLICES;
    rps = std::max<int64_t>(PERM_MIN_SLICE_ROWS, (rps + 15) / 16 * 16);
    P.rps[s] = rps;
    P.slices[s] = (int)((rows[s] + rps - 1) / rps);
    P.ldi[s] = (rows[s] + 3) / 4 * 4;
  }
  P.rep_bytes = 2 * 4 * (P.ldi[0] + P.ldi[1]) + (int64_t)(P.slices[0] + P.slices[1]) * P.cb * 16 * 8;
  const int64_t most = std::max<int64_t>(1, std::min<int64_t>(PERM_MAX_BLOCK, PERM_BLOCK_BYTES / P.rep_bytes));
  P.block = std::min<int64_t>(R, block > 0 ? std::min(block, most) : most);
  P.n_blocks = (R + P.block - 1) / P.block;
  return nullptr;
}

}  // namespace lsspa
