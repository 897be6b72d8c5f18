// Sampled pairwise Shapley interaction index (lsspa_pairs_batch): the two kernels between a batch's lift vectors and
// the per-pair statistics.
//
// For a uniformly random ordering pi of the d players, given that a and b sit at adjacent positions k, k + 1, the set
// S = {pi_0 .. pi_{k-1}} has the interaction index's own weight |S|! (d - 2 - |S|)! / (d - 1)!, so
//     I_ab = E[ v(S + a + b) - v(S + a) - v(S + b) + v(S) | a, b adjacent ].
// Three of the four values are prefixes of pi, the fourth is a prefix of pi with positions k, k + 1 swapped.  Lift vectors
// are indexed by player, so with b = pi_{k+1}
//     Delta_k = lift_pi[b] - lift_pi'[b],   pi' = pi with positions k and k + 1 swapped (b at position k).
// A SAMPLE is three orderings through the ordinary kernels (host_perms.cpp, expand_pair_rows): row 3 s is pi, row 3 s + 1
// pi with positions (0,1), (2,3), .. swapped, row 3 s + 2 pi with positions (1,2), (3,4), .. swapped.  It yields all d - 1
// values Delta_k = row 3 s [b] - row 3 s + 1 + (k & 1) [b], one for each of the d - 1 pairs adjacent in pi.
//
// pairs_delta_kernel: one thread per (sample, position).  Writes Delta [B][d] (entry d - 1 of a row is not used) and the
// inverse ordering pos [B][d] as int16 (d <= 4096).
//
// pairs_accumulate_kernel: owns the table of (count, mean, M2) per unordered pair, kept at [a][b], a < b.  A workgroup
// takes a 64 x 64 tile of pairs: wave w owns rows a = 64 ti + 16 w .. + 15, lane l column b = 64 tj + l.  The positions
// of the tile's 128 players go to LDS in chunks of 256 samples (64 KB).  Every thread walks the samples in sample order;
// where |pos_a - pos_b| = 1 it folds Delta[s][min(pos_a, pos_b)] into its register accumulators by Welford's update, and
// after the batch merges them into the table by Chan's update, once.  No atomics, a fixed order: two runs agree to the
// last bit.  LDS reads: a lane's own pos_b (64 consecutive 16-bit values a wave: two lanes share a dword, 32 banks, no
// conflict) and the wave's 16 pos_a as two 16-byte reads of one address (a broadcast).  The table is written with b
// along the lanes (coalesced rows).
//
// What bounds it: the compare loop, B d^2 / 2 pair-sample tests of a few integer instructions each; the Welford branch
// is taken for 2 / d of them.
#include <algorithm>

#include "kernels.h"

namespace lsspa {

namespace {
constexpr int PT = 64;        // tile edge (players)
constexpr int PROWS = 16;     // rows a thread owns
constexpr int PCHUNK = 256;   // samples staged in LDS at a time
}  // namespace

__global__ __launch_bounds__(256) void pairs_delta_kernel(const double* __restrict__ lifts, int ld,
                                                          const int32_t* __restrict__ perms, int d, int n_samples,
                                                          double* __restrict__ delta, int16_t* __restrict__ pos) {
  const int64_t total = (int64_t)n_samples * d;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
    const int s = (int)(o / d), k = (int)(o - (int64_t)s * d);
    const int32_t* pi = perms + (int64_t)s * d;
    pos[(int64_t)s * d + pi[k]] = (int16_t)k;
    double v = 0.0;
    if (k + 1 < d) {
      const int b = pi[k + 1];
      const double* r0 = lifts + (int64_t)3 * s * ld;
      v = r0[b] - r0[(int64_t)(1 + (k & 1)) * ld + b];
    }
    delta[o] = v;
  }
}

__global__ __launch_bounds__(256) void pairs_accumulate_kernel(const double* __restrict__ delta,
                                                               const int16_t* __restrict__ pos, int d, int n_samples,
                                                               int64_t* __restrict__ t_count,
                                                               double* __restrict__ t_mean, double* __restrict__ t_m2) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (ti > tj) return;
  __shared__ __attribute__((aligned(16))) int16_t sA[PCHUNK][PT];
  __shared__ __attribute__((aligned(16))) int16_t sB[PCHUNK][PT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int a0 = ti * PT + w * PROWS, b = tj * PT + lane;

  int cnt[PROWS];
  double mean[PROWS], m2[PROWS];
#pragma unroll
  for (int k = 0; k < PROWS; ++k) {
    cnt[k] = 0;
    mean[k] = 0.0;
    m2[k] = 0.0;
  }

  for (int c0 = 0; c0 < n_samples; c0 += PCHUNK) {
    const int nc = min(PCHUNK, n_samples - c0);
    __syncthreads();   // the previous chunk has been read
    // players beyond d sit where nobody is their neighbour (and not each other's: the two sides differ)
    for (int r = w; r < nc; r += 4) {
      const int16_t* row = pos + (int64_t)(c0 + r) * d;
      const int ja = ti * PT + lane, jb = tj * PT + lane;
      sA[r][lane] = ja < d ? row[ja] : (int16_t)-30000;
      sB[r][lane] = jb < d ? row[jb] : (int16_t)30000;
    }
    __syncthreads();
    for (int r = 0; r < nc; ++r) {
      const int pb = sB[r][lane];
      const uint4 q0 = *reinterpret_cast<const uint4*>(&sA[r][w * PROWS]);
      const uint4 q1 = *reinterpret_cast<const uint4*>(&sA[r][w * PROWS + 8]);
      const uint32_t qa[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
      const double* drow = delta + (int64_t)(c0 + r) * d;
#pragma unroll
      for (int k = 0; k < PROWS; ++k) {
        const int pa = (int)(int16_t)(k & 1 ? qa[k >> 1] >> 16 : qa[k >> 1] & 0xffffu);
        const int diff = pa - pb;
        if (diff == 1 || diff == -1) {
          const double x = drow[min(pa, pb)];
          cnt[k] += 1;
          const double dl = x - mean[k];
          mean[k] += dl / (double)cnt[k];
          m2[k] += dl * (x - mean[k]);
        }
      }
    }
  }

  if (b >= d) return;
#pragma unroll
  for (int k = 0; k < PROWS; ++k) {
    const int a = a0 + k;
    if (a >= b || cnt[k] == 0) continue;   // a < b < d
    const int64_t at = (int64_t)a * d + b;
    const int64_t n0 = t_count[at];
    if (n0 == 0) {
      t_count[at] = cnt[k];
      t_mean[at] = mean[k];
      t_m2[at] = m2[k];
    } else {
      const double nb = (double)cnt[k], na = (double)n0, n = na + nb;
      const double dl = mean[k] - t_mean[at];
      t_count[at] = n0 + cnt[k];
      t_mean[at] += dl * (nb / n);
      t_m2[at] += m2[k] + dl * dl * (na * nb / n);
    }
  }
}

// phi[j] += sum over the rows of lifts[row][j], rows in order: one thread a player
__global__ __launch_bounds__(256) void pairs_phi_kernel(const double* __restrict__ lifts, int ld, int d, int n_rows,
                                                        double* __restrict__ phi) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= d) return;
  double a = phi[j];
  for (int r = 0; r < n_rows; ++r) a += lifts[(int64_t)r * ld + j];
  phi[j] = a;
}

hipError_t launch_pairs(const double* lifts, int ld, const int32_t* perms, int d, int n_samples, double* delta,
                        int16_t* pos, int64_t* t_count, double* t_mean, double* t_m2, double* phi, hipStream_t st) {
  // (perms are rows the host has validated as permutations of 0 .. d-1: every index below stays inside its buffer)
  if (!lifts || !perms || !delta || !pos || !t_count || !t_mean || !t_m2 || !phi || d < 2 || d > PAIRS_MAX_D ||
      ld < d || n_samples < 1)
    return hipErrorInvalidValue;
  const int64_t total = (int64_t)n_samples * d;
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(pairs_delta_kernel, dim3(blocks), dim3(256), 0, st, lifts, ld, perms, d, n_samples, delta, pos);
  const int nt = (d + PT - 1) / PT;
  hipLaunchKernelGGL(pairs_accumulate_kernel, dim3(nt, nt), dim3(256), 0, st, delta, pos, d, n_samples, t_count, t_mean,
                     t_m2);
  hipLaunchKernelGGL(pairs_phi_kernel, dim3((d + 255) / 256), dim3(256), 0, st, lifts, ld, d, 3 * n_samples, phi);
  return hipGetLastError();
}

}  // namespace lsspa
