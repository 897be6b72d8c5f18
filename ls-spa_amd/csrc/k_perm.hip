// Permutation test of the exact attribution (lsspa_perm_run; DESIGN.md, "Permutation test"): the kernels between the
// device-resident rows of a side and the shared-elimination enumerations of k_multi.hip / k_multi_groups.hip.  fp64
// throughout.
//
// Replicate r permutes y by pi_r (host_perms.cpp: perm_indices, a pure function of (seed, r, side, n)).  G, H and
// ||y_test||^2 do not depend on pi; what does is the p-vector
//   C[r][j] = sum_i X[i][j] y[idx[r][i]],   idx[r][i] = pi_r(i)
// of each side: g_r = C / N on the training side, h_r = C on the test side.  For a block of replicates that is one pass
// over X with y gathered on the fly -- the p x Rb corner of the Gram of [X | Y_perm], without Y_perm ever existing.
//
// perm_xty_kernel<CB>.  v_mfma_f64_16x16x4: A one element a lane, lane l holds A[i = l & 15][k = l >> 4]; B likewise
// B[k = l >> 4][j = l & 15]; D four a lane, register v of lane l is D[(l >> 4) + 4 v][l & 15] (tiles.h).  A is X^T -- 16
// features of column block b < CB (CB = ceil(p / 16) <= 4) by 4 rows --, B is 4 rows by 16 replicates of gathered y, D the
// 16 features x 16 replicates of a wave.  A wave takes SIXTEEN rows a step as four matrix steps: in matrix step s lane
// group k = l >> 4 stands for row base + 4 k + s, so that a lane's four rows are adjacent and its four indices are ONE
// 16-byte load of idx[r][base + 4 k ..] (idx is [Rb][ldi], ldi = n rounded up to 4, as the host drew it: per wave
// instruction 64 contiguous bytes of each of the 16 replicates' index rows, and the next step takes the other half of
// the 128-byte line; one 4-byte index a lane would be 16 bytes of 16 lines an instruction).  Which row meets which k
// slot is the same on both operands and a function of the row number alone, so the sums do not depend on it.
// A workgroup is four waves with four different sets of 16 replicates on the SAME row slice: a row of X comes from
// memory once per workgroup and from the first-level cache for the other three waves; y (8 n bytes) is L2-resident.
// Rows beyond the slice and replicates beyond the block contribute exact zeros through clamped addresses: nothing
// outside X, y or idx is read, and an index is clamped to n - 1 before it is used.
// A wave writes its accumulators as they stand to part[slice][set][b][256]; perm_reduce_kernel adds the slices in
// ascending order, scales, and writes [r][p] into the response slots the enumeration reads.  No floating-point atomics;
// the slices are a function of the row count alone, so a replicate's sums do not depend on its block.
//
// Bound: the index stream, 4 n Rb bytes a side (X is re-read from L2 by the ceil(Rb / 64) workgroups of a slice: 128 CB
// bytes a row against 256 bytes of indices), and the latency of the dependent gather behind it -- not the matrix pipe
// (CB matrix instructions per 4 rows and 16 replicates).
#include "kernels.h"
#include "tiles.h"

namespace lsspa {
namespace {

template <int CB>
__global__ __launch_bounds__(256) void perm_xty_kernel(const double* __restrict__ X, const double* __restrict__ y,
                                                       const uint32_t* __restrict__ idx, int64_t n, int64_t ldi,
                                                       int64_t rps, int reps, double* __restrict__ part) {
  constexpr int LDX = 16 * CB;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int set = (int)blockIdx.y * 4 + wave;
  if (set * 16 >= reps) return;                 // the whole wave; the kernel has no barrier
  const int64_t beg = (int64_t)blockIdx.x * rps;
  const int64_t end = beg + rps < n ? beg + rps : n;      // beg < n: the grid has ceil(n / rps) slices
  const bool live = set * 16 + l15 < reps;
  const uint32_t* irow = idx + (int64_t)(live ? set * 16 + l15 : set * 16) * ldi;
  const uint32_t top = (uint32_t)(n - 1);
  d4 acc[CB];
#pragma unroll
  for (int b = 0; b < CB; ++b) acc[b] = Tr<double>::zero();
  for (int64_t base = beg; base < end; base += 16) {
    const int64_t r4 = base + 4 * l4;           // this lane's four rows r4 .. r4 + 3 (beg and rps are multiples of 16)
    const bool any = r4 < end;                  // r4 < end <= n <= ldi, r4 a multiple of 4: the 16 bytes lie inside the row
    const uint4 iv = *reinterpret_cast<const uint4*>(irow + (any ? r4 : beg));
    const uint32_t ii[4] = {iv.x, iv.y, iv.z, iv.w};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bool in = r4 + s < end;
      const int64_t row = in ? r4 + s : beg;
      const uint32_t src = ii[s] < top ? ii[s] : top;
      const double yv = y[src];
      const double bval = (in && live) ? yv : 0.0;
#pragma unroll
      for (int b = 0; b < CB; ++b) {
        const double xv = X[row * LDX + 16 * b + l15];
        acc[b] = Tr<double>::mfma(in ? xv : 0.0, bval, acc[b]);
      }
    }
  }
  const int sets = (reps + 15) / 16;
  double* out = part + (((int64_t)blockIdx.x * sets + set) * CB) * 256;
#pragma unroll
  for (int b = 0; b < CB; ++b)
#pragma unroll
    for (int v = 0; v < 4; ++v) out[b * 256 + v * 64 + lane] = acc[b][v];
}

// out[r][j], j < p, = scale * (sum over the slices, in order, of the partials); feature j = 16 b + i sits in register
// i >> 2 of lane 16 (i & 3) + (r & 15) of set r >> 4
__global__ __launch_bounds__(256) void perm_reduce_kernel(const double* __restrict__ part, int slices, int reps, int cb,
                                                          int p, double scale, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)reps * p) return;
  const int r = (int)(e / p), j = (int)(e - (int64_t)r * p);
  const int sets = (reps + 15) / 16, b = j >> 4, i = j & 15;
  const int64_t at = ((int64_t)(r >> 4) * cb + b) * 256 + (i >> 2) * 64 + (i & 3) * 16 + (r & 15);
  double s = 0.0;
  for (int sl = 0; sl < slices; ++sl) s += part[(int64_t)sl * sets * cb * 256 + at];
  out[e] = s * scale;
}

// Xd[row0 + i][0 .. p-1] = X[i][:], zero up to ldx; yd[row0 + i] = y[i]
template <typename T>
__global__ __launch_bounds__(256) void perm_pack_kernel(const T* __restrict__ X, int64_t ld, const T* __restrict__ y,
                                                        int64_t rows, int p, double* __restrict__ Xd, int ldx,
                                                        double* __restrict__ yd, int64_t row0) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * ldx) return;
  const int64_t i = e / ldx;
  const int j = (int)(e - i * ldx);
  Xd[(row0 + i) * ldx + j] = j < p ? (double)X[i * ld + j] : 0.0;
  if (j == 0) yd[row0 + i] = (double)y[i];
}

// out[r][j] = src[j] for r < reps: the observed g or h of a side that is not permuted, into every slot
__global__ __launch_bounds__(256) void perm_fill_kernel(const double* __restrict__ src, int p, int reps,
                                                        double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)reps * p) return;
  out[e] = src[e % p];
}

template <int CB>
void xty_launch(const PermPlan& P, int side, const double* X, const double* y, const uint32_t* idx, int64_t n, int reps,
                double* part, hipStream_t st) {
  const dim3 grid((unsigned)P.slices[side], (unsigned)((reps + 63) / 64));
  hipLaunchKernelGGL((perm_xty_kernel<CB>), grid, dim3(256), 0, st, X, y, idx, n, P.ldi[side], P.rps[side], reps, part);
}

}  // namespace

hipError_t launch_perm_xty(const PermPlan& P, int side, const double* X, const double* y, const uint32_t* idx, int64_t n,
                           int reps, double* part, hipStream_t st) {
  if (!X || !y || !idx || !part || n < 1 || n >= (1ll << 31) || reps < 1 || reps > PERM_MAX_BLOCK || side < 0 ||
      side > 1 || P.rps[side] < 16 || P.rps[side] % 16 || (int64_t)P.slices[side] != (n + P.rps[side] - 1) / P.rps[side] ||
      P.ldi[side] != (n + 3) / 4 * 4 || P.cb < 1 || P.cb > 4)
    return hipErrorInvalidValue;
  if (P.cb == 1)
    xty_launch<1>(P, side, X, y, idx, n, reps, part, st);
  else if (P.cb == 2)
    xty_launch<2>(P, side, X, y, idx, n, reps, part, st);
  else if (P.cb == 3)
    xty_launch<3>(P, side, X, y, idx, n, reps, part, st);
  else
    xty_launch<4>(P, side, X, y, idx, n, reps, part, st);
  return hipGetLastError();
}

hipError_t launch_perm_reduce(const PermPlan& P, int side, const double* part, int p, int reps, double scale, double* out,
                              hipStream_t st) {
  if (!part || !out || p < 1 || p > GROUPS_MAX_P || reps < 1 || reps > PERM_MAX_BLOCK || side < 0 || side > 1 ||
      P.cb != (p + 15) / 16 || P.slices[side] < 1)
    return hipErrorInvalidValue;
  const int64_t blocks = ((int64_t)reps * p + 255) / 256;
  hipLaunchKernelGGL(perm_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, part, P.slices[side], reps, P.cb, p,
                     scale, out);
  return hipGetLastError();
}

hipError_t launch_perm_pack(const void* X, int64_t ld, const void* y, int64_t rows, int p, int is_f32, double* Xd, int ldx,
                            double* yd, int64_t row0, hipStream_t st) {
  if (!X || !y || !Xd || !yd || rows < 1 || p < 1 || p > GROUPS_MAX_P || ld < p || ldx < p || ldx % 16 || row0 < 0)
    return hipErrorInvalidValue;
  const int64_t blocks = (rows * ldx + 255) / 256;
  if (blocks > (1ll << 31) - 1) return hipErrorInvalidValue;
  if (is_f32)
    hipLaunchKernelGGL(perm_pack_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)X, ld,
                       (const float*)y, rows, p, Xd, ldx, yd, row0);
  else
    hipLaunchKernelGGL(perm_pack_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, st, (const double*)X, ld,
                       (const double*)y, rows, p, Xd, ldx, yd, row0);
  return hipGetLastError();
}

hipError_t launch_perm_fill(const double* src, int p, int reps, double* out, hipStream_t st) {
  if (!src || !out || p < 1 || p > GROUPS_MAX_P || reps < 1) return hipErrorInvalidValue;
  const int64_t blocks = ((int64_t)reps * p + 255) / 256;
  hipLaunchKernelGGL(perm_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, st, src, p, reps, out);
  return hipGetLastError();
}

}  // namespace lsspa
