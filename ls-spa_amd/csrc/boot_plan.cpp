// How a bootstrap run is cut (lsspa_boot_run): row slices of the weighted Gram pass, replicates per block, replicates and
// steps per enumeration launch.  Host code only, no HIP call: lsspa_debug_boot_plan and a stand-alone sanitiser build
// (tools/boot_plan_check.cpp) exercise it without a GPU.
#include "boot_plan.h"

#include <algorithm>

namespace lsspa {

const char* boot_plan(int64_t R, int64_t N, int64_t M, int p, int64_t block, BootPlan& P) {
  P = BootPlan{};
  if (p < 1 || p > BOOT_MAX_P) return "p must be 1 .. 32";
  if (R < 1) return "R must be at least 1";
  if (N < 1 || M < 1 || N >= (1ll << 31) || M >= (1ll << 31)) return "N and M must be 1 .. 2^31 - 1";
  if (block < 0) return "block must be >= 0";
  const int c = p + 1;
  P.cb = (c + 15) / 16;
  P.ldz = 16 * P.cb;
  P.pairs = P.cb * (P.cb + 1) / 2;
  P.rpw = P.cb <= 2 ? 4 : 2;          // accumulators a wave holds: rpw * pairs * 4 doubles a lane (<= 96 registers)
  const int64_t rows[2] = {N, M};
  for (int s = 0; s < 2; ++s) {
    // a slice: at least BOOT_MIN_SLICE_ROWS rows, at most BOOT_MAX_SLICES of them -- a function of the rows alone, so
    // that a replicate's sums do not depend on how many replicates share its block
    int64_t rps = (rows[s] + BOOT_MAX_SLICES - 1) / BOOT_MAX_SLICES;
    rps = std::max<int64_t>(BOOT_MIN_SLICE_ROWS, (rps + 3) / 4 * 4);
    P.rps[s] = rps;
    P.slices[s] = (int)((rows[s] + rps - 1) / rps);
  }
  const int q = p < BOOT_LOW ? p : BOOT_LOW;
  const uint64_t n_high = 1ull << (p - q);
  P.units = std::min<uint64_t>(n_high, BOOT_UNITS);
  P.per = n_high / P.units;
  // per replicate: weights of both sides (8 bytes a row: fp64 weights; counts take half), the Gram partials of both
  // sides, the enumeration's partial table, and the small per-replicate matrices (S, G, H, ... < 8 c^2 doubles)
  P.rep_bytes = 8 * (N + M) + (int64_t)(P.slices[0] + P.slices[1]) * P.pairs * 256 * 8 +
                (int64_t)P.units * c * 8 + 8ll * c * c * 8;
  int64_t most = std::max<int64_t>(1, std::min<int64_t>(BOOT_MAX_BLOCK, BOOT_BLOCK_BYTES / P.rep_bytes));
  P.block = std::min<int64_t>(R, block > 0 ? std::min(block, most) : most);
  P.n_blocks = (R + P.block - 1) / P.block;
  P.enum_reps = std::max<int64_t>(1, std::min<int64_t>(P.block, (int64_t)(BOOT_SUBSETS_PER_LAUNCH / P.units)));
  P.steps = std::max<uint64_t>(1, BOOT_SUBSETS_PER_LAUNCH / (P.units * (uint64_t)P.enum_reps));
  P.steps = std::min<uint64_t>(P.steps, P.per);
  return nullptr;
}

}  // namespace lsspa
