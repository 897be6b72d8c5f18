// Sampled attribution over GROUPS of columns (lsspa_set_players): the fold of a batch's lift vectors [rows][p] into
// group lifts [samples][g].
//
// The Shapley value of group k is the mean, over orderings of the groups, of the summed lifts of k's columns when the
// ordering is expanded to a column ordering with the baseline first and every group's columns contiguous
// (tests/test_groups_host.py, fact 2).  The gather / Cholesky / lift kernels run on the expanded orderings unchanged;
// this kernel is the one step between their output and everything that follows (statistics, history, estimator), all
// of which then work in dimension g.
//
//   out[s][k] = 1/per * sum over r < per of ( sum over j in cols[off[k] .. off[k+1]) of lifts[s per + r][j] )
//
// per = 1: one row a sample (a plain ordering, or an antithetical pair the lift kernels have averaged already);
// per = 2: rows 2 s and 2 s + 1 are the sample's two orderings, run unpaired (a baseline rules the kernels' paired
// form out: the reversed group ordering still starts with the baseline).  One thread per (sample, group); a group's
// columns are added in ascending column order, the two rows one after the other: a fixed order, no atomics, so two
// runs agree to the last bit.
//
// What bounds it: memory.  It reads rows * p doubles once (a group's columns are one run of the CSR; neighbouring
// threads read neighbouring groups' columns of the same row, which the lift kernel has just written -- 2 MB for 256
// orderings at p = 1000, L2-resident) and writes samples * g.  No LDS, no scratch, a handful of registers.
#include <algorithm>

#include "kernels.h"

namespace lsspa {

__global__ __launch_bounds__(256) void fold_players_kernel(const double* __restrict__ lifts, int p, int per,
                                                           const int32_t* __restrict__ off,
                                                           const int32_t* __restrict__ cols, int g, int n_samples,
                                                           double* __restrict__ out) {
  const int64_t total = (int64_t)n_samples * g;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
    const int s = (int)(o / g), k = (int)(o - (int64_t)s * g);
    const int c0 = off[k], c1 = off[k + 1];
    const double* row = lifts + (int64_t)s * per * p;
    double a = 0.0;
    for (int c = c0; c < c1; ++c) a += row[cols[c]];
    if (per == 2) {
      double b = 0.0;
      for (int c = c0; c < c1; ++c) b += row[p + cols[c]];
      a = 0.5 * (a + b);
    }
    out[o] = a;
  }
}

hipError_t launch_fold_players(const double* lifts, int p, int per, const int32_t* off, const int32_t* cols, int g,
                               int n_samples, double* out, hipStream_t st) {
  // (off and cols are the library's own tables: player_map_build has checked that every column index is in 0 .. p-1)
  if (!lifts || !off || !cols || !out || p < 1 || g < 1 || g > p || n_samples < 1 || (per != 1 && per != 2))
    return hipErrorInvalidValue;
  const int64_t total = (int64_t)n_samples * g;
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(fold_players_kernel, dim3(blocks), dim3(256), 0, st, lifts, p, per, off, cols, g, n_samples, out);
  return hipGetLastError();
}

}  // namespace lsspa
