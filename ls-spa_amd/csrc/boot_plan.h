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
  int64_t enum_reps;       // replicates one enumeration launch takes (units * enum_reps <= BOOT_SUBSETS_PER_LAUNCH)
  uint64_t units, per, steps;   // enumeration: units per replicate, high subsets per unit, steps per launch
};
constexpr int64_t BOOT_BLOCK_BYTES = 256ll << 20;   // what the replicates of one block may take together
constexpr int64_t BOOT_MAX_BLOCK = 1024;
constexpr int64_t BOOT_MIN_SLICE_ROWS = 256, BOOT_MAX_SLICES = 128;
constexpr uint64_t BOOT_UNITS = 8192, BOOT_SUBSETS_PER_LAUNCH = 1ull << 20;   // those of the enumerations' host path
// Host code only (no HIP call): nullptr, or what is wrong with the arguments.  block = 0: as many replicates as
// BOOT_BLOCK_BYTES holds (at most BOOT_MAX_BLOCK); a larger request is cut to that.
const char* boot_plan(int64_t R, int64_t N, int64_t M, int p, int64_t block, BootPlan& P);
constexpr int BOOT_MAX_P = 32, BOOT_LOW = 6;   // SUBSETS_MAX_P and the enumeration's low features (k_subsets.hip)

}  // namespace lsspa
