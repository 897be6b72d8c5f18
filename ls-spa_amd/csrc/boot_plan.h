// How a bootstrap run is cut (lsspa_boot_run, k_boot.hip): plain host declarations, no HIP header, so that boot_plan.cpp
// also builds by itself with a host compiler (tools/boot_plan_check.cpp: the sanitiser run of the planner).
#pragma once
#include <stdint.h>

namespace lsspa {

struct BootPlan {
  int cb, ldz, pairs;      // 16-column blocks of Z, its row stride, cb (cb + 1) / 2 block pairs (upper block triangle)
  int rpw;                 // replicates one wave carries through its rows (4 waves a workgroup)
  int64_t rps[2];          // rows per slice, train / test: a multiple of 4, a function of the side's rows alone
  int slices[2];           // row slices, train / test (the last one may be ragged)
  int64_t rep_bytes;       // device bytes one replicate of a block takes: weights, Gram partials, enumeration partials
  int64_t block, n_blocks; // replicates per block (the last block may hold fewer), blocks
  int64_t enum_reps;       // replicates one enumeration launch takes: units * enum_reps <= BOOT_SUBSETS_PER_LAUNCH; the
                           // interaction planners: units * enum_reps * steps <= that, enum_reps <= BOOT_MAX_BLOCK and a
                           // table of at most BOOT_INTER_TABLE_BYTES (below)
  uint64_t units, per, steps;   // enumeration: units per replicate, high subsets per unit, steps per launch
  int64_t table_bytes;     // the interaction planners: the enumeration's partial table, kept once beside the block (else 0)
};
constexpr int64_t BOOT_BLOCK_BYTES = 256ll << 20;   // what the replicates of one block may take together
constexpr int64_t BOOT_MAX_BLOCK = 1024;
constexpr int64_t BOOT_MIN_SLICE_ROWS = 256, BOOT_MAX_SLICES = 128;
constexpr uint64_t BOOT_UNITS = 8192, BOOT_SUBSETS_PER_LAUNCH = 1ull << 20;   // those of the enumerations' host path
// Host code only (no HIP call): nullptr, or what is wrong with the arguments.  block = 0: as many replicates as
// BOOT_BLOCK_BYTES holds (at most BOOT_MAX_BLOCK); a larger request is cut to that.
const char* boot_plan(int64_t R, int64_t N, int64_t M, int p, int64_t block, BootPlan& P);
constexpr int BOOT_MAX_P = 32, BOOT_LOW = 6;   // SUBSETS_MAX_P and the enumeration's low features (k_subsets.hip)
// The bootstrap of the best-subset selection (lsspa_boot_best_run): boot_plan's cut with the enumeration's table holding,
// per (unit, size), a value, a mask and a found flag -- 16 bytes an entry against the 8 of a sum, counted in rep_bytes
// like boot_plan's: block rep_bytes <= BOOT_BLOCK_BYTES, or block = 1.  units enum_reps steps <= 2^20, and per <=
// BOOT_BEST_MAX_PER, the size classes subsets_best_kernel holds (it is for p <= 32 over BOOT_UNITS units).  The winner
// of a total order depends on no cut, which is therefore chosen for speed: steps as the one-problem call cuts a unit
// (min(per, 2^20 / units)), then enum_reps = what such a launch has left, at most the block, at least 1.
constexpr uint64_t BOOT_BEST_MAX_PER = 1ull << 13;
const char* boot_best_plan(int64_t R, int64_t N, int64_t M, int p, int64_t block, BootPlan& P);
// The bootstrap over groups of columns (lsspa_boot_groups_run): g groups over p <= 64 columns, of which gh are high, nb
// columns the baseline and ql the low groups' (GroupLayout, kernels.h).  c = p + 1 <= 65 columns of Z: cb up to 5; the
// slices are boot_plan's for the same rows; units, per, steps cut the 2^gh high subsets as the one-problem grouped
// enumeration cuts them (BOOT_GROUPS_WORK_PER_LAUNCH / rows^2 subsets a launch): a function of the layout alone, since
// the cut of `per` into launches shows in the bits.  enum_reps replicates share a launch, within that work bound and
// 2^20 workgroups; the enumeration's partial table is g + 1 wide.
const char* boot_groups_plan(int64_t R, int64_t N, int64_t M, int p, int g, int gh, int nb, int ql, int64_t block,
                             BootPlan& P);
constexpr int BOOT_GROUPS_MAX_P = 64, BOOT_GROUPS_MAX_G = 32;   // GROUPS_MAX_P, GROUPS_MAX_G (k_groups.hip)
constexpr uint64_t BOOT_GROUPS_WORK_PER_LAUNCH = 1ull << 26;    // that of lsspa_groups_shapley's host path
// The bootstrap of the best-subset selection over groups (lsspa_boot_groups_best_run): boot_groups_plan's arguments,
// Gram side, units and per, with the enumeration's table holding, per (unit, size), a value, a mask and a found flag --
// 16 bytes an entry, units (g + 1) 16 bytes a replicate, counted in rep_bytes: block rep_bytes <= BOOT_BLOCK_BYTES, or
// block = 1.  per <= BOOT_GROUPS_BEST_MAX_PER always (the size classes groups_best_kernel holds; asserted).  The winner
// of a total order depends on no cut of a unit's steps into launches, and a workgroup computes each u(S) whole: the cut
// is chosen for speed.  steps: the one-problem call's (min(per, max(1, work bound / rows^2 / units))); enum_reps: what
// such a launch leaves -- units enum_reps steps rows^2 <= BOOT_GROUPS_WORK_PER_LAUNCH (unless one step of one replicate
// is already more) and units enum_reps <= 2^20 workgroups --, at most the block, at least 1.
constexpr uint64_t BOOT_GROUPS_BEST_MAX_PER = 1ull << 18;       // 2^(GROUPS_BEST_CLASSES - 1) (kernels.h)
const char* boot_groups_best_plan(int64_t R, int64_t N, int64_t M, int p, int g, int gh, int nb, int ql, int64_t block,
                                  BootPlan& P);

// The bootstrap of the interaction values (lsspa_boot_interactions_run, lsspa_boot_groups_interactions_run): the plans
// above with the enumeration's partial table inter_cols(d) = d (d + 3) / 2 + 2 wide, d = p or g players -- 37 MB a
// replicate at d = 32.  The accounting differs for that reason:
//   - the table is kept for the enum_reps replicates of ONE enumeration launch, not for the block: table_bytes =
//     enum_reps units inter_cols(d) 8, and rep_bytes holds everything else a replicate takes (its row of column sums
//     included).  block rep_bytes + table_bytes <= BOOT_BLOCK_BYTES, or block = 1;
//   - units, per, steps are the one-problem interaction call's own cut, a function of the players alone (ungrouped:
//     steps = min(per, max(1, BOOT_SUBSETS_PER_LAUNCH / units)); grouped: boot_groups_plan's) and never of R, block or
//     enum_reps, since the cut of `per` into launches shows in the bits;
//   - enum_reps fills what a launch of `steps` steps leaves: units enum_reps steps <= 2^20 (grouped: and the work bound
//     BOOT_GROUPS_WORK_PER_LAUNCH), a table of at most BOOT_INTER_TABLE_BYTES, at most the block, at least 1.
// Everything of the Gram side (cb .. slices) is that of boot_plan / boot_groups_plan for the same rows.
constexpr int64_t BOOT_INTER_TABLE_BYTES = 64ll << 20;
inline int boot_inter_cols(int d) { return d + 2 + d + d * (d - 1) / 2; }   // subsets_inter_cols (k_subsets.hip)
const char* boot_inter_plan(int64_t R, int64_t N, int64_t M, int p, int64_t block, BootPlan& P);
const char* boot_groups_inter_plan(int64_t R, int64_t N, int64_t M, int p, int g, int gh, int nb, int ql, int64_t block,
                                   BootPlan& P);

// The bootstrap of the SAMPLED attribution (lsspa_boot_lift_run; k_boot.hip, launch_small_problems): p <= 127, c = p + 1
// <= 128 columns of Z, cb up to 8.  The Gram side is boot_plan's for the same rows (cb, ldz, pairs, rps, slices: the
// slices a function of the side's rows alone); gram_form 0 is boot_gram_kernel<CB, RPW> (cb <= 5, rpw as above), 1 the
// wide form of cb = 6 .. 8, in which the four waves of a workgroup share the rows AND the replicate and divide the block
// pairs among themselves (rpw = 1: one replicate a workgroup).  A replicate's problem is written at the ordering
// kernels' stride: rows of BOOT_LIFT_LD doubles.  The orderings are one set for all replicates, n_samples samples of
// per = 1 or 2 (antithetical) orderings; a lift launch is a grid (orderings, replicates):
//   - samples_per_launch = min(n_samples, BOOT_LIFT_ORD / per): a function of n_samples and antithetical alone, never of
//     R, first or block -- the running (n, mean, M2) of a replicate is merged once per cut, so the cut shows in the bits;
//   - reps_per_launch fills what such a launch leaves: orderings x replicates <= BOOT_LIFT_GRID_REG workgroups of the
//     register-resident kernel (lift_form 0, p + 1 <= 112), <= BOOT_LIFT_GRID_LDS of the LDS-resident one (lift_form 1,
//     one workgroup a compute unit), and raw lifts [orderings][replicates][p] of at most BOOT_LIFT_RAW_BYTES; it does not
//     show in the bits (a workgroup computes one (ordering, replicate) whole);
//   - block rep_bytes <= BOOT_BLOCK_BYTES (or block = 1), block <= BOOT_MAX_BLOCK; the raw lifts stand beside the block.
// launches: lift launches of the whole run; raw_bytes: those of the largest launch.
struct BootLiftPlan {
  int cb, ldz, pairs, gram_form, rpw;
  int64_t rps[2];
  int slices[2];
  int64_t rep_bytes, block, n_blocks;
  int lift_form;
  int64_t samples_per_launch, ord_per_launch, reps_per_launch, sample_cuts, launches, raw_bytes;
};
constexpr int BOOT_LIFT_MAX_P = 127, BOOT_LIFT_LD = 128;      // CV_LIFT_MAX_P, CV_LIFT_LD (kernels.h)
constexpr int64_t BOOT_LIFT_ORD = 256;
constexpr int64_t BOOT_LIFT_GRID_REG = 1 << 16, BOOT_LIFT_GRID_LDS = 1 << 13;
constexpr int64_t BOOT_LIFT_RAW_BYTES = 256ll << 20;
// d: the dimension of a sample (p, or the groups of a player map, 1 <= d <= p); block as boot_plan's
const char* boot_lift_plan(int64_t R, int64_t N, int64_t M, int p, int d, int64_t n_samples, int antithetical,
                           int64_t block, BootLiftPlan& P);

// The permutation test (lsspa_perm_run, k_perm.hip): X of a side lives on the device as [n][ldx], ldx = 16 cb, cb =
// ceil(p / 16) <= 4; a block of replicates is one gathered X^T y pass per permuted side into per-slice partial sums
// [slice][ceil(block / 16)][cb][256].  A slice is at least PERM_MIN_SLICE_ROWS rows, a multiple of 16, at most
// PERM_MAX_SLICES of them: a function of the side's rows alone, so that a replicate's sums do not depend on its block.
// ldi: the row stride of the index table [block][ldi], n rounded up to 4 (the kernel reads 16 bytes a lane).
// rep_bytes: what one replicate of a block takes -- its index rows of both sides, twice (the next block's are drawn and
// uploaded while this one runs; the same again in pinned host memory), and its partials; block = 0: as many replicates
// as PERM_BLOCK_BYTES holds, at most PERM_MAX_BLOCK (a larger request is cut to that).
struct PermPlan {
  int cb, ldx;
  int64_t rps[2], ldi[2];
  int slices[2];
  int64_t rep_bytes, block, n_blocks;
};
constexpr int64_t PERM_BLOCK_BYTES = 256ll << 20, PERM_MAX_BLOCK = 1024;
constexpr int64_t PERM_MIN_SLICE_ROWS = 256, PERM_MAX_SLICES = 128;
constexpr int PERM_MAX_P = 64;                  // GROUPS_MAX_P; without groups the enumeration takes p <= 32
const char* perm_plan(int64_t R, int64_t N, int64_t M, int p, int64_t block, PermPlan& P);

}  // namespace lsspa
