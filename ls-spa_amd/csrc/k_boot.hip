// Bootstrap of the exact attribution (lsspa_boot_run; DESIGN.md, "Bootstrap confidence intervals"): the kernels between
// the device-resident rows Z = [X | y] of a side and the enumeration of k_subsets.hip.  fp64 throughout.
//
// A bootstrap replicate draws n rows with replacement; its reduced problem is the WEIGHTED Gram
//   S[r] = sum_i w[r][i] z_i z_i^T,   w[r][i] = how often row i was drawn
// -- or any non-negative weights the caller hands in.  For a block of replicates that is one pass over Z.
//
// Counts (boot_counts_kernel).  Draw t of replicate r on side s (0 train, 1 test) is a pure function of (seed, r, s, t):
// Philox4x32-10 with key = (seed low, seed high) and counter = (t / 4, s, r low, r high); output word k serves draw
// t = 4 (t / 4) + k and the row is  (uint64(word) * n) >> 32,  n < 2^31 (exact integer arithmetic).  Row i is then drawn
// with probability (ceil or floor of 2^32 (i + 1) / n - 2^32 i / n) / 2^32: a bias of at most n / 2^32 relative to 1 / n.
// Counts are added with integer atomics, which commute: the table is the same on every run.
//
// Weighted Gram (boot_gram_kernel).  v_mfma_f64_16x16x4: A = one element a lane, lane l holds A[i = l & 15][k = l >> 4];
// B likewise B[k = l >> 4][j = l & 15]; D four a lane, register v of lane l is D[(l >> 4) + 4 v][l & 15] (tiles.h).  A wave
// takes four rows a step: lane l loads z[row + (l >> 4)][16 b + (l & 15)] for the cb 16-column blocks b of Z -- as it
// stands the B operand of block b -- and the row's weight of each of its RPW replicates; the A operand w z is formed in
// registers.  Block pairs bi <= bj only (S is symmetric): RPW * cb (cb + 1) / 2 accumulators of four doubles (RPW = 4, 4,
// 2, 1, 1 at cb = 1 .. 5; cb = 4, 5 are the bootstrap over groups of columns, p <= 64).  A workgroup
// is four waves with four different sets of replicates on the SAME rows, so a row of Z comes from memory once per
// workgroup and from the first-level cache for the other three waves; the workgroups of one row slice that belong to the
// other replicates of the block find it in L2 (a slice is at most a few hundred KB).  Rows beyond the slice get weight 0
// and a clamped address; nothing outside Z or the weight table is read.
// A wave writes its accumulators as they stand to part[slice][r][pair][256]; boot_reduce_kernel adds the slices in
// order and unfolds the layout, taking (i, j) and (j, i) from the one element computed for i <= j: S is exactly
// symmetric, there are no floating-point atomics, and since the slices are a function of the rows alone a replicate's
// sums do not depend on the block it was in.
#include "kernels.h"
#include "philox.h"
#include "tiles.h"

namespace lsspa {
namespace {

__global__ __launch_bounds__(256) void boot_counts_kernel(uint64_t seed, uint64_t r0, int side, int64_t n,
                                                          uint32_t* __restrict__ cnt) {
  const int64_t t4 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (4 * t4 >= n) return;
  const uint64_t r = r0 + blockIdx.y;
  uint32_t w[4];
  philox4x32_10((uint32_t)t4, (uint32_t)side, (uint32_t)r, (uint32_t)(r >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
  uint32_t* row = cnt + (int64_t)blockIdx.y * n;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (4 * t4 + k < n) atomicAdd(row + (((uint64_t)w[k] * (uint64_t)n) >> 32), 1u);   // index < n
}

template <int CB, int RPW>
__global__ __launch_bounds__(256) void boot_gram_kernel(const double* __restrict__ Z, int64_t n, int64_t rps,
                                                        const uint32_t* __restrict__ cnt,
                                                        const double* __restrict__ wt, int reps,
                                                        double* __restrict__ part) {
  constexpr int LDZ = 16 * CB, PAIRS = CB * (CB + 1) / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int r0 = ((int)blockIdx.y * 4 + wave) * RPW;
  if (r0 >= reps) return;                       // the whole wave; the kernel has no barrier
  const int64_t beg = (int64_t)blockIdx.x * rps;
  const int64_t end = beg + rps < n ? beg + rps : n;      // beg < n: the grid has ceil(n / rps) slices
  int64_t wrow[RPW];
  bool live[RPW];
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    live[k] = r0 + k < reps;
    wrow[k] = (int64_t)(live[k] ? r0 + k : r0) * n;
  }
  d4 acc[RPW][PAIRS];
#pragma unroll
  for (int k = 0; k < RPW; ++k)
#pragma unroll
    for (int e = 0; e < PAIRS; ++e) acc[k][e] = Tr<double>::zero();
  for (int64_t base = beg; base < end; base += 4) {
    const bool in = base + l4 < end;
    const int64_t row = in ? base + l4 : beg;
    double z[CB], w[RPW];
#pragma unroll
    for (int b = 0; b < CB; ++b) {
      const double v = Z[row * LDZ + 16 * b + l15];
      z[b] = in ? v : 0.0;
    }
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
      const double v = cnt ? (double)cnt[wrow[k] + row] : wt[wrow[k] + row];
      w[k] = (in && live[k]) ? v : 0.0;
    }
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
      int e = 0;
#pragma unroll
      for (int bi = 0; bi < CB; ++bi) {
        const double a = w[k] * z[bi];
#pragma unroll
        for (int bj = bi; bj < CB; ++bj, ++e) acc[k][e] = Tr<double>::mfma(a, z[bj], acc[k][e]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    if (!live[k]) continue;
    double* out = part + (((int64_t)blockIdx.x * reps + r0 + k) * PAIRS) * 256;
#pragma unroll
    for (int e = 0; e < PAIRS; ++e)
#pragma unroll
      for (int v = 0; v < 4; ++v) out[e * 256 + v * 64 + lane] = acc[k][e][v];
  }
}

__global__ __launch_bounds__(256) void boot_wsum_kernel(const uint32_t* __restrict__ cnt,
                                                        const double* __restrict__ wt, int64_t n,
                                                        double* __restrict__ wsum) {
  __shared__ double red[256];
  const int64_t off = (int64_t)blockIdx.x * n;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) s += cnt ? (double)cnt[off + i] : wt[off + i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) wsum[blockIdx.x] = red[0];
}

// S[r][i][j], i, j <= p, from the element the Gram pass computed for (min, max): block pair (bi, bj) of the upper block
// triangle, row-major; inside a block row a = 4 v + (l >> 4), column b = l & 15
__global__ __launch_bounds__(256) void boot_reduce_kernel(const double* __restrict__ part, int slices, int reps,
                                                          int cb, int c, double* __restrict__ S) {
  const int r = blockIdx.x, pairs = cb * (cb + 1) / 2;
  for (int e = threadIdx.x; e < c * c; e += 256) {
    const int i = e / c, j = e - i * c;
    const int a = i < j ? i : j, b = i < j ? j : i;
    const int bi = a >> 4, bj = b >> 4;
    const int pr = bi * cb - bi * (bi - 1) / 2 + (bj - bi);
    const int ia = a & 15, ib = b & 15;
    const int64_t at = (int64_t)pr * 256 + (ia >> 2) * 64 + (ia & 3) * 16 + ib;
    double s = 0.0;
    for (int sl = 0; sl < slices; ++sl) s += part[((int64_t)sl * reps + r) * pairs * 256 + at];
    S[(int64_t)r * c * c + e] = s;
  }
}

__global__ __launch_bounds__(256) void boot_finalize_kernel(const double* __restrict__ S_tr,
                                                            const double* __restrict__ S_te,
                                                            const double* __restrict__ wsum_tr, int p, double reg,
                                                            double* __restrict__ G, double* __restrict__ g,
                                                            double* __restrict__ H, double* __restrict__ h,
                                                            double* __restrict__ inv_yy) {
  const int r = blockIdx.x, c = p + 1;
  const double* A = S_tr + (int64_t)r * c * c;
  const double* T = S_te + (int64_t)r * c * c;
  const double W = wsum_tr[r];
  for (int e = threadIdx.x; e < p * p; e += 256) {
    const int i = e / p, j = e - i * p;
    G[(int64_t)r * p * p + e] = A[i * c + j] / W + (i == j ? reg : 0.0);
    H[(int64_t)r * p * p + e] = T[i * c + j];
  }
  if ((int)threadIdx.x < p) {
    g[(int64_t)r * p + threadIdx.x] = A[threadIdx.x * c + p] / W;
    h[(int64_t)r * p + threadIdx.x] = T[threadIdx.x * c + p];
  }
  if (threadIdx.x == 0) inv_yy[r] = 1.0 / T[p * c + p];
}

template <typename T>
__global__ __launch_bounds__(256) void boot_pack_kernel(const T* __restrict__ X, int64_t ld, const T* __restrict__ y,
                                                        int64_t rows, int p, double* __restrict__ Z, int ldz,
                                                        int64_t row0) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * ldz) return;
  const int64_t i = e / ldz;
  const int j = (int)(e - i * ldz);
  double v = 0.0;
  if (j < p)
    v = (double)X[i * ld + j];
  else if (j == p)
    v = (double)y[i];
  Z[(row0 + i) * ldz + j] = v;
}

// The wide form, cb = 6 .. 8 (the bootstrap of the sampled attribution, p + 1 = 81 .. 128 columns): a wave cannot hold
// the cb (cb + 1) / 2 accumulators of even one replicate beside its operands (36 x 4 doubles at cb = 8), so the four
// waves of a workgroup share the rows AND the replicate and divide the block pairs among themselves: pair e (row-major
// over bi <= bj, boot_reduce_kernel's numbering) belongs to wave e & 3, which keeps it in accumulator e >> 2 -- at most
// 9 accumulators of four doubles a wave.  Every wave loads the row's cb blocks once per four rows (the first wave from
// memory, the others from the first-level cache) and forms the A operand w z in registers.  The accumulators go to the
// same part[slice][r][pair][256] as they stand: boot_reduce_kernel sums and unfolds them unchanged.  No barrier, no
// LDS, no atomics; rows beyond the slice get weight 0 and a clamped address.  W is the wave, a template parameter so
// that every accumulator index is a constant (wide_wave picks the instantiation by the wave's number, a scalar).
template <int CB, int W>
__device__ __forceinline__ void boot_gram_wide_wave(const double* __restrict__ Z, int64_t n, int64_t beg, int64_t end,
                                                    const uint32_t* __restrict__ cnt, const double* __restrict__ wt,
                                                    int64_t wrow, double* __restrict__ out, int lane) {
  constexpr int LDZ = 16 * CB, PAIRS = CB * (CB + 1) / 2, MINE = (PAIRS - W + 3) / 4;
  const int l15 = lane & 15, l4 = lane >> 4;
  d4 acc[MINE];
#pragma unroll
  for (int e = 0; e < MINE; ++e) acc[e] = Tr<double>::zero();
  for (int64_t base = beg; base < end; base += 4) {
    const bool in = base + l4 < end;
    const int64_t row = in ? base + l4 : beg;
    double z[CB];
#pragma unroll
    for (int b = 0; b < CB; ++b) {
      const double v = Z[row * LDZ + 16 * b + l15];
      z[b] = in ? v : 0.0;
    }
    const double wv = cnt ? (double)cnt[wrow + row] : wt[wrow + row];
    const double w = in ? wv : 0.0;
    int e = 0;
#pragma unroll
    for (int bi = 0; bi < CB; ++bi) {
      const double a = w * z[bi];
#pragma unroll
      for (int bj = bi; bj < CB; ++bj, ++e)
        if ((e & 3) == W) acc[e >> 2] = Tr<double>::mfma(a, z[bj], acc[e >> 2]);
    }
  }
#pragma unroll
  for (int k = 0; k < MINE; ++k)
#pragma unroll
    for (int v = 0; v < 4; ++v) out[(int64_t)(4 * k + W) * 256 + v * 64 + lane] = acc[k][v];
}

template <int CB>
__global__ __launch_bounds__(256) void boot_gram_wide_kernel(const double* __restrict__ Z, int64_t n, int64_t rps,
                                                             const uint32_t* __restrict__ cnt,
                                                             const double* __restrict__ wt, int reps,
                                                             double* __restrict__ part) {
  constexpr int PAIRS = CB * (CB + 1) / 2;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int r = blockIdx.y;                               // r < reps: the grid has reps rows
  const int64_t beg = (int64_t)blockIdx.x * rps;
  const int64_t end = beg + rps < n ? beg + rps : n;      // beg < n: the grid has ceil(n / rps) slices
  const int64_t wrow = (int64_t)r * n;
  double* out = part + (((int64_t)blockIdx.x * reps + r) * PAIRS) * 256;
  switch (wave) {
    case 0: boot_gram_wide_wave<CB, 0>(Z, n, beg, end, cnt, wt, wrow, out, lane); break;
    case 1: boot_gram_wide_wave<CB, 1>(Z, n, beg, end, cnt, wt, wrow, out, lane); break;
    case 2: boot_gram_wide_wave<CB, 2>(Z, n, beg, end, cnt, wt, wrow, out, lane); break;
    default: boot_gram_wide_wave<CB, 3>(Z, n, beg, end, cnt, wt, wrow, out, lane); break;
  }
}

// boot_finalize_kernel's expressions into the layout the ordering kernels of k_small.hip read (launch_small_problems):
// rows of LD doubles, a replicate's matrices LD x LD apart; aug: the diagonals of the two augmented rows by
// launch_cv_lift_finalize's rule (2 ||y_train||^2 / W + 1, 2 ||y_test||^2 + 1).  Entries beyond column p - 1 and row
// p - 1 are not written: the caller has zeroed the buffers once.
__global__ __launch_bounds__(256) void boot_lift_finalize_kernel(const double* __restrict__ S_tr,
                                                                 const double* __restrict__ S_te,
                                                                 const double* __restrict__ wsum_tr, int p, double reg,
                                                                 double* __restrict__ G, double* __restrict__ g,
                                                                 double* __restrict__ H, double* __restrict__ h,
                                                                 double* __restrict__ inv_yy, double* __restrict__ aug) {
  constexpr int LD = BOOT_LIFT_LD;
  const int r = blockIdx.x, c = p + 1;
  const double* A = S_tr + (int64_t)r * c * c;
  const double* T = S_te + (int64_t)r * c * c;
  const double W = wsum_tr[r];
  for (int e = threadIdx.x; e < p * p; e += 256) {
    const int i = e / p, j = e - i * p;
    G[((int64_t)r * LD + i) * LD + j] = A[i * c + j] / W + (i == j ? reg : 0.0);
    H[((int64_t)r * LD + i) * LD + j] = T[i * c + j];
  }
  if ((int)threadIdx.x < p) {
    g[(int64_t)r * LD + threadIdx.x] = A[threadIdx.x * c + p] / W;
    h[(int64_t)r * LD + threadIdx.x] = T[threadIdx.x * c + p];
  }
  if (threadIdx.x == 0) {
    inv_yy[r] = 1.0 / T[p * c + p];
    aug[2 * r] = 2.0 * (A[p * c + p] / W) + 1.0;
    aug[2 * r + 1] = 2.0 * T[p * c + p] + 1.0;
  }
}

// One thread per (replicate r of the launch, player k).  raw [ordering][reps][p] is a lift launch's output.  Sample s's
// entry: the ordering's lift (no map), or the sum of group k's columns in ascending column order from 0.0 per ordering
// (cv_lift_fold_kernel's rule and bits); a pair's is 0.5 a + 0.5 b of its two orderings' entries.  Welford over the
// launch's samples in sample order, then one Chan merge into the replicate's running (mean, M2) of n_old samples
// (multi_lift_stats_kernel's expressions).  samples (may be NULL): the entries themselves, [reps][n_s][d].
__global__ __launch_bounds__(256) void boot_lift_stats_kernel(const double* __restrict__ raw, int p, int reps, int per,
                                                              const int32_t* __restrict__ off,
                                                              const int32_t* __restrict__ cols, int d, int n_s,
                                                              double n_old, double* __restrict__ mean,
                                                              double* __restrict__ M2, double* __restrict__ samples) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= (int64_t)reps * d) return;
  const int r = (int)(o / d);
  const int k = (int)(o - (int64_t)r * d);
  const int c0 = off ? off[k] : 0, c1 = off ? off[k + 1] : 0;
  double mb = 0.0, qb = 0.0;
  for (int s = 0; s < n_s; ++s) {
    double e[2] = {0.0, 0.0};
    for (int q = 0; q < per; ++q) {
      const double* row = raw + (((int64_t)s * per + q) * reps + r) * p;
      if (off) {
        double a = 0.0;
        for (int c = c0; c < c1; ++c) a += row[cols[c]];
        e[q] = a;
      } else {
        e[q] = row[k];
      }
    }
    const double x = per == 2 ? 0.5 * e[0] + 0.5 * e[1] : e[0];
    if (samples) samples[((int64_t)r * n_s + s) * d + k] = x;
    const double dl = x - mb;
    mb += dl / (double)(s + 1);
    qb += dl * (x - mb);
  }
  if (n_old == 0.0) {
    mean[o] = mb;
    M2[o] = qb;
  } else {
    const double nbd = (double)n_s, n = n_old + nbd;
    const double dl = mb - mean[o];
    mean[o] += dl * (nbd / n);
    M2[o] += qb + dl * dl * (n_old * nbd / n);
  }
}

template <int CB, int RPW>
void gram_launch(const BootPlan& P, int side, const double* Z, int64_t n, const uint32_t* cnt, const double* wt,
                 int reps, double* part, hipStream_t st) {
  const dim3 grid((unsigned)P.slices[side], (unsigned)((reps + 4 * RPW - 1) / (4 * RPW)));
  hipLaunchKernelGGL((boot_gram_kernel<CB, RPW>), grid, dim3(256), 0, st, Z, n, P.rps[side], cnt, wt, reps, part);
}

}  // namespace

hipError_t launch_boot_counts(uint64_t seed, uint64_t r0, int side, int64_t n, int reps, uint32_t* cnt,
                              hipStream_t st) {
  if (!cnt || n < 1 || n >= (1ll << 31) || reps < 1 || reps > 65535 || side < 0 || side > 1)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(cnt, 0, sizeof(uint32_t) * (size_t)n * reps, st);
  if (e != hipSuccess) return e;
  const int64_t calls = (n + 3) / 4;
  hipLaunchKernelGGL(boot_counts_kernel, dim3((unsigned)((calls + 255) / 256), (unsigned)reps), dim3(256), 0, st, seed,
                     r0, side, n, cnt);
  return hipGetLastError();
}

hipError_t launch_boot_gram(const BootPlan& P, int side, const double* Z, int64_t n, const uint32_t* cnt,
                            const double* wt, int reps, double* part, hipStream_t st) {
  if (!Z || !part || (cnt == nullptr) == (wt == nullptr) || n < 1 || reps < 1 || side < 0 || side > 1 ||
      P.rps[side] < 4 || P.rps[side] % 4 || (int64_t)P.slices[side] != (n + P.rps[side] - 1) / P.rps[side] ||
      P.ldz != 16 * P.cb || reps > 65535 * 4)
    return hipErrorInvalidValue;
  if (P.cb == 1 && P.rpw == 4)
    gram_launch<1, 4>(P, side, Z, n, cnt, wt, reps, part, st);
  else if (P.cb == 2 && P.rpw == 4)
    gram_launch<2, 4>(P, side, Z, n, cnt, wt, reps, part, st);
  else if (P.cb == 3 && P.rpw == 2)
    gram_launch<3, 2>(P, side, Z, n, cnt, wt, reps, part, st);
  else if (P.cb == 4 && P.rpw == 1)            // the bootstrap over groups: p + 1 = 49 .. 64 columns
    gram_launch<4, 1>(P, side, Z, n, cnt, wt, reps, part, st);
  else if (P.cb == 5 && P.rpw == 1)            // p = 64
    gram_launch<5, 1>(P, side, Z, n, cnt, wt, reps, part, st);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_boot_wsum(const uint32_t* cnt, const double* wt, int64_t n, int reps, double* wsum, hipStream_t st) {
  if ((cnt == nullptr) == (wt == nullptr) || !wsum || n < 1 || reps < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(boot_wsum_kernel, dim3((unsigned)reps), dim3(256), 0, st, cnt, wt, n, wsum);
  return hipGetLastError();
}

hipError_t launch_boot_reduce(const BootPlan& P, int side, const double* part, int p, int reps, double* S,
                              hipStream_t st) {
  if (!part || !S || p < 1 || p > GROUPS_MAX_P || reps < 1 || side < 0 || side > 1 || P.cb != (p + 16) / 16 ||
      P.slices[side] < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(boot_reduce_kernel, dim3((unsigned)reps), dim3(256), 0, st, part, P.slices[side], reps, P.cb,
                     p + 1, S);
  return hipGetLastError();
}

hipError_t launch_boot_finalize(const double* S_tr, const double* S_te, const double* wsum_tr, int p, double reg,
                                int reps, double* G, double* g, double* H, double* h, double* inv_yy,
                                hipStream_t st) {
  if (!S_tr || !S_te || !wsum_tr || !G || !g || !H || !h || !inv_yy || p < 1 || p > GROUPS_MAX_P || reps < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(boot_finalize_kernel, dim3((unsigned)reps), dim3(256), 0, st, S_tr, S_te, wsum_tr, p, reg, G, g,
                     H, h, inv_yy);
  return hipGetLastError();
}

hipError_t launch_boot_pack(const void* X, int64_t ld, const void* y, int64_t rows, int p, int is_f32, double* Z,
                            int ldz, int64_t row0, hipStream_t st) {
  if (!X || !y || !Z || rows < 1 || p < 1 || p > GROUPS_MAX_P || ld < p || ldz < p + 1 || row0 < 0)
    return hipErrorInvalidValue;
  const int64_t blocks = (rows * ldz + 255) / 256;
  if (blocks > (1ll << 31) - 1) return hipErrorInvalidValue;
  if (is_f32)
    hipLaunchKernelGGL(boot_pack_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)X, ld,
                       (const float*)y, rows, p, Z, ldz, row0);
  else
    hipLaunchKernelGGL(boot_pack_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, st, (const double*)X, ld,
                       (const double*)y, rows, p, Z, ldz, row0);
  return hipGetLastError();
}

// ---- the bootstrap of the sampled attribution (lsspa_boot_lift_*): c = p + 1 up to 128 columns --------------------------
// The launchers above keep their p <= GROUPS_MAX_P; these are their siblings for p <= BOOT_LIFT_MAX_P on the same kernels.
hipError_t launch_boot_lift_gram(const BootLiftPlan& L, int side, const double* Z, int64_t n, const uint32_t* cnt,
                                 const double* wt, int reps, double* part, hipStream_t st) {
  if (L.cb < 1 || L.cb > 8 || L.gram_form != (L.cb >= 6) || side < 0 || side > 1) return hipErrorInvalidValue;
  if (!L.gram_form) {                  // the existing instantiations, through their launcher
    BootPlan P{};
    P.cb = L.cb;
    P.ldz = L.ldz;
    P.pairs = L.pairs;
    P.rpw = L.rpw;
    P.rps[side] = L.rps[side];
    P.slices[side] = L.slices[side];
    return launch_boot_gram(P, side, Z, n, cnt, wt, reps, part, st);
  }
  if (!Z || !part || (cnt == nullptr) == (wt == nullptr) || n < 1 || n >= (1ll << 31) || reps < 1 || reps > 65535 ||
      L.rps[side] < 4 || L.rps[side] % 4 || (int64_t)L.slices[side] != (n + L.rps[side] - 1) / L.rps[side] ||
      L.ldz != 16 * L.cb || L.pairs != L.cb * (L.cb + 1) / 2)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)L.slices[side], (unsigned)reps);
  if (L.cb == 6)
    hipLaunchKernelGGL(boot_gram_wide_kernel<6>, grid, dim3(256), 0, st, Z, n, L.rps[side], cnt, wt, reps, part);
  else if (L.cb == 7)
    hipLaunchKernelGGL(boot_gram_wide_kernel<7>, grid, dim3(256), 0, st, Z, n, L.rps[side], cnt, wt, reps, part);
  else
    hipLaunchKernelGGL(boot_gram_wide_kernel<8>, grid, dim3(256), 0, st, Z, n, L.rps[side], cnt, wt, reps, part);
  return hipGetLastError();
}

hipError_t launch_boot_lift_reduce(const BootLiftPlan& L, int side, const double* part, int p, int reps, double* S,
                                   hipStream_t st) {
  if (!part || !S || p < 1 || p > BOOT_LIFT_MAX_P || reps < 1 || side < 0 || side > 1 || L.cb != (p + 16) / 16 ||
      L.slices[side] < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(boot_reduce_kernel, dim3((unsigned)reps), dim3(256), 0, st, part, L.slices[side], reps, L.cb,
                     p + 1, S);
  return hipGetLastError();
}

hipError_t launch_boot_lift_pack(const void* X, int64_t ld, const void* y, int64_t rows, int p, int is_f32, double* Z,
                                 int ldz, int64_t row0, hipStream_t st) {
  if (!X || !y || !Z || rows < 1 || p < 1 || p > BOOT_LIFT_MAX_P || ld < p || ldz < p + 1 || row0 < 0)
    return hipErrorInvalidValue;
  const int64_t blocks = (rows * ldz + 255) / 256;
  if (blocks > (1ll << 31) - 1) return hipErrorInvalidValue;
  if (is_f32)
    hipLaunchKernelGGL(boot_pack_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)X, ld,
                       (const float*)y, rows, p, Z, ldz, row0);
  else
    hipLaunchKernelGGL(boot_pack_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, st, (const double*)X, ld,
                       (const double*)y, rows, p, Z, ldz, row0);
  return hipGetLastError();
}

hipError_t launch_boot_lift_finalize(const double* S_tr, const double* S_te, const double* wsum_tr, int p, double reg,
                                     int reps, double* G, double* g, double* H, double* h, double* inv_yy, double* aug,
                                     hipStream_t st) {
  if (!S_tr || !S_te || !wsum_tr || !G || !g || !H || !h || !inv_yy || !aug || p < 1 || p > BOOT_LIFT_MAX_P || reps < 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(boot_lift_finalize_kernel, dim3((unsigned)reps), dim3(256), 0, st, S_tr, S_te, wsum_tr, p, reg, G,
                     g, H, h, inv_yy, aug);
  return hipGetLastError();
}

hipError_t launch_boot_lift_stats(const double* raw, int p, int reps, int per, const int32_t* off, const int32_t* cols,
                                  int d, int n_s, int64_t n_old, double* mean, double* M2, double* samples,
                                  hipStream_t st) {
  // (off and cols are the library's own tables: player_map_build has checked that every column index is in 0 .. p-1)
  if (!raw || !mean || !M2 || p < 1 || p > BOOT_LIFT_MAX_P || reps < 1 || (per != 1 && per != 2) || d < 1 || d > p ||
      (off ? !cols : d != p) || n_s < 1 || n_old < 0)
    return hipErrorInvalidValue;
  const int64_t total = (int64_t)reps * d;
  hipLaunchKernelGGL(boot_lift_stats_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, raw, p, reps, per,
                     off, cols, d, n_s, (double)n_old, mean, M2, samples);
  return hipGetLastError();
}

}  // namespace lsspa
