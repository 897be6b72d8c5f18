// Exact Shapley attribution over GROUPS of columns (g <= 32 groups, p <= 64 columns, an always-included baseline):
// u(S) = v(B + columns of the groups in S) of all 2^g group subsets, never stored, folded into the Shapley sum of the
// group game as it is computed.  fp64 throughout.  k_subsets.hip with "feature" read as "set of columns":
//
//   v(K) = (2 theta_K^T h_K - theta_K^T H_KK theta_K) / ||y_test||^2,  theta_K = G_KK^-1 g_K,  v({}) = 0,
//   phi_k = sum_{S not containing k} w(|S|) (u(S + k) - u(S)),   w(s) = s! (g - 1 - s)! / g!.
//
// Decomposition ("Exact attribution over groups of columns"): the host picks gl LOW groups (the smallest
// ones, while their columns total ql <= 6); the other gh = g - gl groups are HIGH.  One workgroup of four waves owns one
// high subset Hs at a time:
//   1. it compacts [G g] over B + cols(Hs) + low columns into LDS (nk <= 64 rows, nk + 1 columns) and eliminates the
//      pivots of B + cols(Hs) by Gauss-Jordan, in place.  A lane owns a row, a wave every fourth column to the right of
//      the pivot: the columns to its left are never read again, so they are not kept up (half the work of a full
//      sweep), and a column is read and written by one wave only, so a pivot costs one barrier.  That leaves
//      A^-1 [C g] in the pivot rows (A = G over B + cols(Hs), C its coupling to the low columns) and the Schur
//      complement S, g~ in the low block;
//   2. theta over everything is e0 + E theta_T with e0 = [A^-1 g; 0], E = [-A^-1 C; I]: the test side reduces to the
//      (ql+1) x (ql+1) matrix Z = X^T H X and z = X^T h of X = [e0 E] (H read from global memory, a row at a time:
//      H is symmetric, so the lanes of a wave read neighbouring words);
//   3. lane T of the first wave (one lane per subset of the low groups, 2^gl <= 64) masks the rows and columns of S
//      whose group is not in T to the identity and runs the fixed 6 x 6 Cholesky, solves and quadratic form of
//      k_subsets.hip in registers.
// The Shapley sum is that file's too, over groups: with a(K) = w(|K| - 1) u(K), b(K) = w(|K|) u(K),
//   phi_k = sum_{K containing k} (a + b)(K) - sum_K b(K),
// kept per lane, reduced once per launch by fixed butterflies into the unit's row of a partial table [units][g + 1]
// (low groups first, then the high ones, then b) which launch_subsets_reduce sums in fixed order.  No floating-point
// atomics: the result is bitwise the same from call to call.
//
// Pairwise Shapley interaction index between groups (lsspa_groups_interactions, the INTER instantiation of the
// enumeration kernel): k_subsets.hip's sums with players = groups of the layout,
//   I_kl = T0 - T1_k - T1_l + T2_kl,   T0 = sum_K gamma u,   T1_k = sum_{K with k} (beta + gamma) u,
//   T2_kl = sum_{K with k and l} (alpha + 2 beta + gamma) u,
// and a unit's row of the partial table [0 .. g] as above | T0 | T1 [g] | T2 [g (g - 1) / 2] (layout numbering, pairs
// i < j row-major: subsets_inter_cols(g) columns).  Only wave 0 holds values here, and its registers are the scarce ones
// (the 6 x 6 Cholesky), so per step it keeps three sums a lane (for T0, the low groups' T1 and the low-low pairs) and
// hands the rest to all four waves through LDS, under the barrier that ends a step anyway:
//   - dv[T] = (alpha + 2 beta + gamma) u(Hs + T) per lane.  High-low pair (t, j) is the sum over the lanes T with t of the
//     steps with j in hi: wave w, lane T keeps that sum for the eight high groups j = 8 w .. 8 w + 7;
//   - wave 0's sums of the step over T of (beta + gamma) u and of dv.  Both belong to hi alone: the first goes to T1 of
//     the high groups in hi (thread j keeps group j's), the second to the pairs of high groups inside hi, which are
//     dealt over the 256 threads (at most HH = 2 a thread) with their masks built once.
// Every cell of the table is written by one thread, the sums are fixed butterflies and fixed loops: bitwise reproducible.
//
// Owen value (lsspa_groups_owen, the OWEN instantiation of the enumeration kernel): the two-level Shapley value of the
// columns of one group, the target, with the groups as coalition structure.  The players of the launch are those of the
// target's refined game -- the other groups whole (outer players), the target's b columns as singletons (inner players)
// -- and everything above runs on them unchanged; only the weight of a subset K differs, by two counts instead of |K|:
// with r outer and t inner players in K,
//   a(K) = wo(r) wi(t - 1) u(K),  b(K) = wo(r) wi(t) u(K),   wo(r) = r! (g - 1 - r)! / g!,  wi(t) = t! (b - 1 - t)! / b!,
//   Ow_i = sum_{K containing i} (a + b)(K) - sum_K b(K)      for an inner player i
// (the outer players' columns of the table are written too and mean nothing).  t is a popcount of tid and one of hi
// under the two masks of the inner players that the host leaves in GROUPS_TAB_OWEN_LO / _HI of the layout table, r the
// rest of |K|; wo, wi(t - 1), wi(t) are rows 2 .. 4 of GroupArgs::w.  GroupArgs itself is as it was: a field more cost
// an instantiation its registers once already (REPS below).
//
// Best group subset of every size (lsspa_groups_best, groups_best_kernel below): a kernel of its own beside the
// enumeration kernel -- an arg-max cannot be had from its sums -- with the same workgroup, units, steps, load_shared and
// group_values; no Owen weights, and replicates only in its REPS instantiation (the bootstrap of the selection,
// lsspa_boot_groups_best_run: the launch's second grid dimension, like the enumeration kernel's).  What it keeps of u(Hs + T) is, per size k = |Hs| +
// |T| (groups, not columns; size 0 is the baseline alone), the largest value and its subset.  Order: the larger value
// wins, on equal values the numerically smaller mask in the CALLER's numbering (bit k = label k); a subset whose own
// pivots failed -- the workgroup's high ones or the lane's low ones -- is no candidate and NaN never wins (v > best from
// -inf).  The order is total, so the result does not depend on how the work is cut.
//   Running bests: hi = blockIdx.x per + s with per a power of two, so inside a unit the size class of a step is
// popc(s), at most GROUPS_BEST_CLASSES = 19 classes (per <= 2^18: gh <= 31 over 8192 units).  Lane T of wave 0 keeps
// (value, hi) per class in LDS, [class][lane], its own slots only: popc(s) indexes them, no scratch and no unrolled
// chain of 19 branches, and 14.6 KB on top of GrpShared leave the two workgroups a CU that the enumeration kernel's
// registers allow.  groups_layout numbers the high groups in ascending label order, so for a fixed lane ascending hi is
// ascending caller mask: the strict compare keeps the smaller mask of equal values.
//   Merge: at the end of a launch, for every size the unit can hold, the lane translates (hi, T) to the caller's mask
// through GroupLayout::gid (32 bytes by value in the kernel's arguments) -- across lanes the layout's order is not the
// caller's: a low group has a small layout number whatever its label --, wave 0 reduces (value, mask) by a fixed
// butterfly under the total order, and lane 0 merges the winner into the unit's row of the table, values [units][g + 1]
// and (caller mask, found) [units][g + 1][2], with plain loads and stores (one workgroup owns a row, launches are ordered
// by the stream).  launch_subsets_best_reduce then takes the best over the units.  No atomics on the table.
//
// K-fold cross-validation over groups (lsspa_cv_groups_best, groups_cv_best_kernel below): that kernel's sibling, which
// takes every high subset through the K fold problems of k_cv.hip in one step and keeps the best SUM of their values
// per size.  The attribution (lsspa_cv_groups_shapley) needs no kernel of its own: the folds are replicates of the
// enumeration kernel's REPS instantiation.  The T best sums per size (lsspa_cv_groups_top, groups_cv_top_kernel below):
// that kernel's fold-step with groups_top_kernel's lists.
#include "kernels.h"

#include <algorithm>
#include <numeric>

namespace lsspa {
namespace {

constexpr int GQ = GROUPS_LOW_COLS;            // low columns at most: the register-resident Cholesky
constexpr int GP = GROUPS_MAX_P;               // 64
constexpr int GG = GROUPS_MAX_G;               // 32
constexpr int LDM = GP + 1;                    // row stride of the compacted matrix: nk columns and the right-hand side
constexpr int XC = GQ + 1;                     // row stride of X and Y
constexpr int ZC = GQ + 2;                     // row stride of Z: columns 0 .. ql of X^T H X, then X^T h
constexpr int NT = 256;                        // four waves
constexpr int GW = GG / 4;                     // INTER: high groups whose high-low sums one wave keeps (8)
constexpr int GHI = GG - 1;                    // INTER: high groups at most (launch_groups_enum)
constexpr int HH = (GHI * (GHI - 1) / 2 + NT - 1) / NT;   // INTER: pairs of high groups a thread owns at most (2)

struct GrpShared {
  double M[GP * LDM];      // compacted [G g] being eliminated: rows = columns of the subset, odd stride
  double X[GP * XC];       // [e0 E]
  double Y[GP * XC];       // H X
  double Z[XC * ZC];       // X^T H X | X^T h
  double h[GP];
  double gdiag[GP];        // diagonal of G: the pivot scale
  double wa[GG + 1], wb[GG + 1];
  int idx[GP];             // compacted position -> column
  int cols[GP];            // the layout (GroupLayout::tab)
  int colgrp[GP];
  int colin[GP];
  int hsize[GG];
  int lgrp[GQ];
};

// what the INTER instantiation adds (the other one declares none of it)
struct GrpInterShared {
  double w2[3 * (GG + 1)];   // gamma, beta + gamma, alpha + 2 beta + gamma by |K|
  double dv[64];             // the step's (alpha + 2 beta + gamma) u per lane of wave 0
  double se, sd;             // the step's sums over wave 0 of (beta + gamma) u and of dv
};

// what the OWEN instantiation adds (the others declare none of it): the weights by the two counts
struct GrpOwenShared {
  double wo[GG + 1];         // wo(r), r = 0 .. g - 1 outer players
  double wia[GG + 1];        // wi(t - 1), t = 0 .. b inner players (0 at t = 0)
  double wib[GG + 1];        // wi(t) (0 at t = b)
};

__device__ inline double wave_sum(double x) {
  // fixed butterfly, then lane 0's value for everyone: the same order on every call
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return __shfl(x, 0, 64);
}

// wave_sum of one value per low group at once: each by the butterfly above, the chains interleaved -- a shuffle's latency
// is most of a lone wave_sum, and the interactions kernel ends a launch with up to 48 of them a wave
__device__ inline void wave_sum_low(double (&x)[GQ]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int t = 0; t < GQ; ++t) x[t] += __shfl_xor(x[t], o, 64);
  }
}

// Replicates (the bootstrap, k_boot.hip): replicate r = blockIdx.y of a launch has its problem r strides behind the
// launch's, at the dense strides of k_subsets.hip -- G, H: p ld, g, h: p, one 1 / ||y||^2 (GroupArgs::inv_yy_rep) and one
// info word each, part: the table of the replicates before it.  The layout table, the weights and the labels are the
// launch's.  Those are the REPS instantiations (phi-only and INTER, whose row of the table is subsets_inter_cols(g)
// wide); without REPS the replicate is 0 at compile time and the code is what it was before replicates existed (explicit
// stride arguments cost k_subsets.hip its occupancy).
template <bool REPS>
__device__ inline int64_t rep_offset(int64_t stride) { return REPS ? (int64_t)blockIdx.y * stride : 0; }

// u(Hs + T) of this thread's low subset T = tid (0 for threads >= 2^gl).  Enters and leaves with the workgroup in
// step: every shared array it writes is free when it is called and is read by nobody after it returns.
template <bool REPS>
__device__ double group_values(GrpShared& sh, const GroupArgs& a, uint64_t hi, int tid, bool& bad) {
  const int p = a.p, ql = a.ql, nb = a.nb, gh = a.gh;
  const int wv = tid >> 6, lane = tid & 63;
  const double* Gr = a.G + rep_offset<REPS>((int64_t)p * a.ldg);
  const double* gr = a.g + rep_offset<REPS>(p);
  // pivots of this subset: the baseline, then the columns of the high groups of hi in layout order
  const int myg = (tid < p) ? sh.colgrp[tid] : -1;
  int nhs = nb, off = 0;
  for (int j = 0; j < gh; ++j) {
    if (j == myg) off = nhs;
    if ((hi >> j) & 1ull) nhs += sh.hsize[j];
  }
  if (tid < p) {
    if (tid < nb)
      sh.idx[tid] = sh.cols[tid];
    else if (tid >= p - ql)
      sh.idx[nhs + tid - (p - ql)] = sh.cols[tid];
    else if ((hi >> myg) & 1ull)
      sh.idx[off + sh.colin[tid]] = sh.cols[tid];
  }
  const int nk = nhs + ql;    // columns of B + Hs + low: rows of M; column nk of M is the right-hand side
  __syncthreads();
  for (int i = wv; i < nk; i += 4) {
    const int ci = sh.idx[i];
    for (int j = lane; j <= nk; j += 64)
      sh.M[i * LDM + j] = (j < nk) ? Gr[(int64_t)ci * a.ldg + sh.idx[j]] : gr[ci];
  }
  __syncthreads();
  // Gauss-Jordan on the pivots 0 .. nhs-1, columns right of the pivot only.  Column j belongs to wave (j - k - 1) % 4
  // of step k: its lanes read the pivot row's entry before lane k overwrites it (one instruction stream), column k
  // itself is not written in step k, and the barrier separates the steps.
  for (int k = 0; k < nhs; ++k) {
    const double d = sh.M[k * LDM + k];
    if (!(d > a.piv_tol * sh.gdiag[sh.idx[k]])) bad = true;
    const double inv = 1.0 / d;
    if (lane < nk) {
      const double mik = sh.M[lane * LDM + k];
      for (int j = k + 1 + wv; j <= nk; j += 4) {
        const double mkj = sh.M[k * LDM + j] * inv;
        const double mij = sh.M[lane * LDM + j];
        sh.M[lane * LDM + j] = (lane == k) ? mkj : mij - mik * mkj;
      }
    }
    __syncthreads();
  }
  // X = [e0 E] over the nk compacted columns (columns 0 .. ql of X)
  const int nc = ql + 1;
  for (int e = tid; e < nk * nc; e += NT) {
    const int i = e / nc, c = e - i * nc;
    double x;
    if (i < nhs)
      x = (c == 0) ? sh.M[i * LDM + nk] : -sh.M[i * LDM + nhs + c - 1];
    else
      x = (c - 1 == i - nhs) ? 1.0 : 0.0;
    sh.X[i * XC + c] = x;
  }
  __syncthreads();
  // Y = H X: lane = row i, wave wv takes columns wv and wv + 4; H_ib is read as H_bi, a contiguous run of row b
  if (lane < nk && wv < nc) {
    const bool two = wv + 4 < nc;
    const double* Hc = a.H + rep_offset<REPS>((int64_t)p * a.ldh) + sh.idx[lane];
    double s0 = 0.0, s1 = 0.0;
    for (int b = 0; b < nk; ++b) {
      const double hv = Hc[(int64_t)sh.idx[b] * a.ldh];
      s0 += hv * sh.X[b * XC + wv];
      if (two) s1 += hv * sh.X[b * XC + wv + 4];
    }
    sh.Y[lane * XC + wv] = s0;
    if (two) sh.Y[lane * XC + wv + 4] = s1;
  }
  __syncthreads();
  if (tid < nc * (nc + 1)) {
    const int c = tid / (nc + 1), c2 = tid - c * (nc + 1);
    double s = 0.0;
    if (c2 < nc)
      for (int i = 0; i < nk; ++i) s += sh.X[i * XC + c] * sh.Y[i * XC + c2];
    else
      for (int i = 0; i < nk; ++i) s += sh.X[i * XC + c] * sh.h[sh.idx[i]];
    sh.Z[c * ZC + (c2 < nc ? c2 : GQ + 1)] = s;
  }
  __syncthreads();
  // lane T of the first wave: theta_T = S_TT^-1 g~_T with every column whose group is outside T masked to the identity
  double v = 0.0;
  if (tid < (1 << a.gl)) {
    bool in[GQ];
#pragma unroll
    for (int t = 0; t < GQ; ++t) in[t] = (t < ql) && ((tid >> sh.lgrp[t]) & 1);
    double L[GQ][GQ], y[GQ];
#pragma unroll
    for (int t = 0; t < GQ; ++t) {
      const double mt = (t < ql) ? sh.M[(nhs + t) * LDM + nk] : 0.0;
      y[t] = in[t] ? mt : 0.0;
#pragma unroll
      for (int s = 0; s <= t; ++s) {
        const double ms = (t < ql) ? sh.M[(nhs + t) * LDM + nhs + s] : 0.0;
        L[t][s] = (in[t] && in[s]) ? ms : (s == t ? 1.0 : 0.0);
      }
    }
#pragma unroll
    for (int j = 0; j < GQ; ++j) {
      double d = L[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
      if (in[j] && !(d > a.piv_tol * sh.gdiag[sh.idx[nhs + j]])) bad = true;
      const double r = 1.0 / sqrt(d);
      L[j][j] = d * r;
#pragma unroll
      for (int i = j + 1; i < GQ; ++i) {
        double s = L[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
        L[i][j] = s * r;
      }
    }
#pragma unroll
    for (int i = 0; i < GQ; ++i) {
      double s = y[i];
#pragma unroll
      for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
      y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = GQ - 1; i >= 0; --i) {
      double s = y[i];
#pragma unroll
      for (int k = i + 1; k < GQ; ++k) s -= L[k][i] * y[k];
      y[i] = s / L[i][i];                 // theta_T (exactly 0 outside T)
    }
    double f = 2.0 * sh.Z[GQ + 1] - sh.Z[0];
#pragma unroll
    for (int t = 0; t < GQ; ++t) {
      if (t < ql) {
        double u = 2.0 * (sh.Z[(1 + t) * ZC + GQ + 1] - sh.Z[(1 + t) * ZC]);
#pragma unroll
        for (int s = 0; s < GQ; ++s)
          if (s < ql) u -= sh.Z[(1 + t) * ZC + 1 + s] * y[s];
        f += y[t] * u;
      }
    }
    if constexpr (REPS)
      v = f * a.inv_yy_rep[blockIdx.y];
    else
      v = f * a.inv_yy;
  }
  return v;
}

template <bool REPS>
__device__ void load_shared(GrpShared& sh, const GroupArgs& a, int tid) {
  const int p = a.p;
  if (tid < p) {
    sh.h[tid] = a.h[rep_offset<REPS>(p) + tid];
    sh.gdiag[tid] = a.G[rep_offset<REPS>((int64_t)p * a.ldg) + (int64_t)tid * a.ldg + tid];
    sh.cols[tid] = a.tab[GROUPS_TAB_COLS + tid];
    sh.colgrp[tid] = a.tab[GROUPS_TAB_COLGRP + tid];
    sh.colin[tid] = a.tab[GROUPS_TAB_COLIN + tid];
  }
  if (tid < GG) sh.hsize[tid] = a.tab[GROUPS_TAB_HSIZE + tid];
  if (tid < GQ) sh.lgrp[tid] = a.tab[GROUPS_TAB_LGRP + tid];
  if (tid <= a.ng) {
    sh.wa[tid] = a.w[tid];
    sh.wb[tid] = a.w[GG + 1 + tid];
  }
  for (int e = tid; e < XC * ZC; e += NT) sh.Z[e] = 0.0;   // rows / columns beyond ql stay 0
  __syncthreads();
}

// column of pair (i, j), i < j, among the g (g - 1) / 2 pairs of a row of the interactions table
__device__ inline int pair_col(int g, int i, int j) { return i * (2 * g - i - 1) / 2 + (j - i - 1); }

// INTER: the interaction sums T0, T1, T2 beside phi's (lsspa_groups_interactions); a row of part is then
// subsets_inter_cols(g) wide.  Everything of the phi-only instantiation is in both, unchanged.  REPS: the launch's second
// grid dimension is the replicate (rep_offset above).  OWEN (phi-only, one problem): the weights of the Owen value of a
// target group's columns (the header); nothing else differs.
template <bool INTER, bool REPS = false, bool OWEN = false>
__global__ __launch_bounds__(NT) void groups_enum_kernel(GroupArgs a, uint64_t s0, uint64_t s1) {
  static_assert(!OWEN || (!INTER && !REPS), "the Owen weights exist for phi of one problem only");
  __shared__ GrpShared sh;
  __shared__ GrpInterShared si;                // INTER only: never referenced, hence not allocated, otherwise
  __shared__ GrpOwenShared so;                 // OWEN only, likewise
  const int tid = threadIdx.x;
  const int ng = a.ng, gl = a.gl, gh = a.gh;
  // INTER with REPS: the replicate's strides go into the arguments once, here, and the code below is the one-problem
  // kernel's (RO = false) -- offsets formed at every use, as the phi-only REPS instantiation forms them, cost this one
  // scalar registers it does not have and sent it to scratch
  constexpr bool RO = REPS && !INTER;
  if constexpr (REPS && INTER) {
    const int64_t r = blockIdx.y;
    a.G += r * a.p * a.ldg;
    a.H += r * a.p * a.ldh;
    a.g += r * a.p;
    a.h += r * a.p;
    a.info += r;
    a.part += r * gridDim.x * (ng + 2 + ng + ng * (ng - 1) / 2);
    a.inv_yy = a.inv_yy_rep[r];
  }
  load_shared<RO>(sh, a, tid);
  double acc[GG];
#pragma unroll
  for (int j = 0; j < GG; ++j) acc[j] = 0.0;
  double c_own = 0.0, b_own = 0.0;
  // INTER only (dead code otherwise)
  double hl[GW], hh[HH];
  uint32_t hm[HH];
  double g_own = 0.0, e_own = 0.0, d_own = 0.0, t1h = 0.0;
  if constexpr (INTER) {
    for (int e = tid; e < 3 * (GG + 1); e += NT) si.w2[e] = a.w[2 * (GG + 1) + e];
#pragma unroll
    for (int j = 0; j < GW; ++j) hl[j] = 0.0;
    // pair number e = tid + NT r of the gh (gh - 1) / 2 pairs j1 < j2 of high groups, as a mask over hi.  A slot without
    // a pair gets bit 31, which no hi contains: hi < 2^gh and gh <= 31 (launch_groups_enum refuses more; groups_layout
    // never makes more, for gh = 32 means g = 32 without a low group, every group of 7 columns or more, and
    // 32 x 7 > 64 = GROUPS_MAX_P).
#pragma unroll
    for (int r = 0; r < HH; ++r) {
      hh[r] = 0.0;
      int rem = tid + NT * r, j1 = 0;
      while (j1 < gh - 1 && rem >= gh - 1 - j1) {
        rem -= gh - 1 - j1;
        ++j1;
      }
      hm[r] = (j1 < gh - 1) ? ((1u << j1) | (1u << (j1 + 1 + rem))) : 0x80000000u;
    }
    __syncthreads();                           // w2
  }
  // OWEN only: the inner players among the high bits, and this lane's count of them among its low bits (tid)
  uint32_t in_hi = 0;
  int tl = 0;
  if constexpr (OWEN) {
    for (int e = tid; e <= GG; e += NT) {
      so.wo[e] = a.w[2 * (GG + 1) + e];
      so.wia[e] = a.w[3 * (GG + 1) + e];
      so.wib[e] = a.w[4 * (GG + 1) + e];
    }
    in_hi = (uint32_t)a.tab[GROUPS_TAB_OWEN_HI];
    tl = __popc(tid & a.tab[GROUPS_TAB_OWEN_LO]);
    __syncthreads();                           // the three tables
  }
  bool bad = false;
  const bool live = tid < (1 << gl);
  const int kt = __popc(tid);
  for (uint64_t s = s0; s < s1; ++s) {
    const uint64_t hi = (uint64_t)blockIdx.x * a.per + s;
    const double v = group_values<RO>(sh, a, hi, tid, bad);
    if (live) {
      const int k = __popcll(hi) + kt;
      double wab, wb;
      if constexpr (OWEN) {
        const int t = tl + __popc((uint32_t)hi & in_hi);     // gh <= 31 (launch_groups_owen)
        const double w = so.wo[k - t];
        wab = w * (so.wia[t] + so.wib[t]);
        wb = w * so.wib[t];
      } else {
        wab = sh.wa[k] + sh.wb[k];
        wb = sh.wb[k];
      }
      const double c = wab * v;
      c_own += c;
      b_own += wb * v;
#pragma unroll
      for (int j = 0; j < GG; ++j)
        if (j < gh && ((hi >> j) & 1ull)) acc[j] += c;
    }
    if constexpr (INTER) {
      // si.dv, se, sd: written here, after the last barrier of group_values; read below, before the first barrier of the
      // next step's group_values
      if (tid < 64) {
        double e = 0.0, d = 0.0;
        if (live) {
          const int k = __popcll(hi) + kt;
          e = si.w2[GG + 1 + k] * v;
          d = si.w2[2 * (GG + 1) + k] * v;
          g_own += si.w2[k] * v;
          e_own += e;
          d_own += d;
        }
        si.dv[tid] = d;
        const double se = wave_sum(e), sd = wave_sum(d);
        if (tid == 0) {
          si.se = se;
          si.sd = sd;
        }
      }
    }
    __syncthreads();
    if constexpr (INTER) {
      const uint32_t h32 = (uint32_t)hi;       // gh <= 31
      const double d = si.dv[tid & 63];
      const int jw = (tid >> 6) * GW;
#pragma unroll
      for (int j = 0; j < GW; ++j)
        if ((h32 >> (jw + j)) & 1u) hl[j] += d;          // (bits of hi from gh on are 0)
      if ((h32 >> (tid & 31)) & 1u) t1h += si.se;        // thread j < gh: T1 of high group j (the others' is not read)
      const double sd = si.sd;
#pragma unroll
      for (int r = 0; r < HH; ++r)
        if ((h32 & hm[r]) == hm[r]) hh[r] += sd;
    }
  }
  const int cols = INTER ? ng + 2 + ng + ng * (ng - 1) / 2 : ng + 1;
  if (tid < 64) {     // the live lanes all sit in the first wave
    double* part = a.part + (rep_offset<RO>(gridDim.x) + (int64_t)blockIdx.x) * cols;
#pragma unroll
    for (int t = 0; t < GQ; ++t) {
      if (t < gl) {
        const double tot = wave_sum((live && ((tid >> t) & 1)) ? c_own : 0.0);
        if (tid == 0) part[t] += tot;
      }
    }
#pragma unroll
    for (int j = 0; j < GG; ++j) {
      if (j < gh) {
        const double tot = wave_sum(acc[j]);
        if (tid == 0) part[gl + j] += tot;
      }
    }
    const double tb = wave_sum(b_own);
    if (tid == 0) part[ng] += tb;
  }
  if constexpr (INTER) {
    double* part = a.part + (int64_t)blockIdx.x * cols;
    double* t1 = part + ng + 2;
    double* t2 = t1 + ng;
    const int lane = tid & 63;
    const bool lane_live = lane < (1 << gl);
    double x[GQ];
    if (tid < 64) {
      const double t0 = wave_sum(g_own);
      if (tid == 0) part[ng + 1] += t0;
#pragma unroll
      for (int t = 0; t < GQ; ++t) x[t] = (lane_live && ((lane >> t) & 1)) ? e_own : 0.0;
      wave_sum_low(x);
#pragma unroll
      for (int t = 0; t < GQ; ++t)
        if (tid == 0 && t < gl) t1[t] += x[t];
#pragma unroll
      for (int u = 0; u < GQ - 1; ++u) {          // low-low pairs (u, t), u < t
        if (u < gl - 1) {
#pragma unroll
          for (int t = 0; t < GQ; ++t)
            x[t] = (t > u && lane_live && ((lane >> u) & 1) && ((lane >> t) & 1)) ? d_own : 0.0;
          wave_sum_low(x);
#pragma unroll
          for (int t = u + 1; t < GQ; ++t)
            if (tid == 0 && t < gl) t2[pair_col(ng, u, t)] += x[t];
        }
      }
    }
    if (tid < gh) t1[gl + tid] += t1h;            // (gh <= 31: tid & 31 above was tid)
    const int jw = (tid >> 6) * GW;
#pragma unroll
    for (int j = 0; j < GW; ++j) {
      if (jw + j < gh) {                          // the same for the whole wave: high-low pairs (t, gl + jw + j)
#pragma unroll
        for (int t = 0; t < GQ; ++t) x[t] = (lane_live && ((lane >> t) & 1)) ? hl[j] : 0.0;
        wave_sum_low(x);
#pragma unroll
        for (int t = 0; t < GQ; ++t)
          if (lane == 0 && t < gl) t2[pair_col(ng, t, gl + jw + j)] += x[t];
      }
    }
#pragma unroll
    for (int r = 0; r < HH; ++r) {                // high-high pairs: every thread holds the sums of its own
      if (hm[r] != 0x80000000u) {
        const int j1 = __ffs((int)hm[r]) - 1, j2 = 31 - __clz((int)hm[r]);
        t2[pair_col(ng, gl + j1, gl + j2)] += hh[r];
      }
    }
  }
  if (__any(bad) && (tid & 63) == 0) atomicOr(a.info + rep_offset<RO>(1), 1);
}

// ---- best group subset of every size (lsspa_groups_best; the header) ----
constexpr int GBS = GROUPS_BEST_CLASSES;       // size classes of a unit: popc(s), s < per <= 2^(GBS - 1)

struct GroupIds {
  uint8_t id[GG];                              // GroupLayout::gid: the caller's label of the layout's group r
};

struct GrpBestShared {
  double v[GBS * 64];      // [class][lane of wave 0]: the lane's largest u of the class so far (-inf: none)
  uint32_t h[GBS * 64];    // and the hi that gave it
  int gid[GG];
};

// k_subsets.hip's total order (best_merge, wave_best there): the larger value, on equal values the smaller mask; "no
// candidate" is v = -inf, which loses against every candidate
__device__ inline void best_merge(double& v, uint32_t& mask, double bv, uint32_t bmask) {
  const bool take = bv > v || (bv == v && bmask < mask);
  v = take ? bv : v;
  mask = take ? bmask : mask;
}

__device__ inline void wave_best(double& v, uint32_t& mask) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const uint32_t om = (uint32_t)__shfl_xor((int)mask, o, 64);
    best_merge(v, mask, ov, om);
  }
}

// a.part [units][g + 1] (values), bm [units][g + 1][2] (caller mask, found): unit u's best subset of every size so far;
// a launch merges its own into them (found = 0: no candidate yet).  One workgroup owns a row, launches are ordered by
// the stream: plain loads and stores.
// REPS (the bootstrap of the selection over groups, lsspa_boot_groups_best_run): replicate blockIdx.y reads its own
// problem, 1 / ||y||^2 and info word (rep_offset; load_shared<true>, group_values<true>) and merges into its own rows of
// the tables [reps][units][g + 1] and [reps][units][g + 1][2]; layout, weights and ids are the launch's.  The order is
// total, so a replicate's result depends neither on the cut of `per` into launches nor on the replicates beside it.
// Offsets formed at every use, as the phi-only REPS enumeration forms them: this kernel keeps its running bests in LDS,
// not in registers, and has the room (no scratch, the one-problem instantiation's registers).  Without REPS
// the code is what it was.
template <bool REPS = false>
__global__ __launch_bounds__(NT) void groups_best_kernel(GroupArgs a, uint64_t s0, uint64_t s1, GroupIds ids,
                                                         uint32_t* __restrict__ bm) {
  __shared__ GrpShared sh;
  __shared__ GrpBestShared sb;
  const int tid = threadIdx.x;
  const int ng = a.ng, gl = a.gl, gh = a.gh;
  const bool live = tid < (1 << gl);           // wave 0 only (gl <= 6)
  if (tid < GG) sb.gid[tid] = ids.id[tid];
  if (live) {
    for (int j = 0; j < GBS; ++j) {            // the lane's own slots: nobody else reads or writes them
      sb.v[j * 64 + tid] = -__builtin_huge_val();
      sb.h[j * 64 + tid] = 0u;
    }
  }
  load_shared<REPS>(sh, a, tid);               // (ends with a barrier: gid)
  bool any_bad = false;
  for (uint64_t s = s0; s < s1; ++s) {
    const uint64_t hi = (uint64_t)blockIdx.x * a.per + s;
    bool bad = false;                          // this subset's own pivots: the high ones the workgroup's, the low ones the lane's
    const double v = group_values<REPS>(sh, a, hi, tid, bad);
    any_bad |= bad;
    // a lane sees the subsets of a class in ascending hi, which is ascending caller mask (groups_layout numbers the
    // high groups in ascending label order): the strict compare keeps the smaller one, and NaN never wins
    if (live && !bad) {
      const int e = __popcll(s) * 64 + tid;    // popc(s) < GBS: launch_groups_best
      if (v > sb.v[e]) {
        sb.v[e] = v;
        sb.h[e] = (uint32_t)hi;                // gh <= 31
      }
    }
    __syncthreads();
  }
  if (tid < 64) {
    double* rv = a.part + (rep_offset<REPS>(gridDim.x) + (int64_t)blockIdx.x) * (ng + 1);
    uint32_t* rm = bm + (rep_offset<REPS>(gridDim.x) + (int64_t)blockIdx.x) * (ng + 1) * 2;
    // the sizes this unit can hold: popc(unit) + popc(s) + popc(T), s < per (a power of two), T < 2^gl
    const int ncls = __popcll(a.per - 1) + 1;
    const int k0 = __popc(blockIdx.x), k1 = min(ng, k0 + ncls - 1 + gl);
    const int base = k0 + __popc(tid);         // |S| of this lane's class 0
    uint32_t low = 0u;                         // the lane's low groups in the caller's numbering
    for (int r = 0; r < gl; ++r)
      if ((tid >> r) & 1) low |= 1u << sb.gid[r];
    for (int k = k0; k <= k1; ++k) {
      const int j = k - base;
      double v = -__builtin_huge_val();
      uint32_t mask = 0u;
      if (live && j >= 0 && j < ncls) {
        v = sb.v[j * 64 + tid];
        const uint32_t h = sb.h[j * 64 + tid];
        mask = low;
        for (int r = 0; r < gh; ++r)
          if ((h >> r) & 1u) mask |= 1u << sb.gid[gl + r];
      }
      wave_best(v, mask);                      // over caller masks: across lanes the layout's order is not the caller's
      if (tid == 0 && v > -__builtin_huge_val()) {
        if (rm[2 * k + 1] != 0u) best_merge(v, mask, rv[k], rm[2 * k]);
        rv[k] = v;
        rm[2 * k] = mask;
        rm[2 * k + 1] = 1u;
      }
    }
  }
  if (__any(any_bad) && (tid & 63) == 0) atomicOr(a.info + rep_offset<REPS>(1), 1);
}

// ---- best group subset of every size by the K-fold cross-validated value (lsspa_cv_groups_best) ----
// groups_best_kernel<false>'s sibling: the same workgroup, units, steps and launches, running bests per class popc(s) in
// GrpBestShared, merge, table layout and launch_subsets_best_reduce.  What is compared is not one problem's u(S) but
//   u_cv(S) = u_0(S) + u_1(S) + ... + u_{F-1}(S)   (fp64, in this order),
// u_f the value group_values gives for fold problem f: the F reduced problems of k_cv.hip lie one behind the other at the
// dense replicate stride (GroupArgs::inv_yy_rep has their F denominators), and one step takes its high subset through all
// of them before the compare.  A subset is a candidate only if its own pivots passed in EVERY fold; a failed pivot raises
// the info word of the fold it failed in.
//   group_values reads G, g and H of its problem from memory; of the workgroup's LDS only sh.h and sh.gdiag belong to a
// problem.  A fold-step stages fold f's 2 p words into them and runs group_values<false> on fold f's addresses -- the
// same code on other addresses, so u_f has the bits the one-problem kernels give for problem f -- and LDS stays
// GrpShared + GrpBestShared whatever F is: two workgroups a CU, as the sibling's ("K-fold cross-validation
// over groups", has the alternatives).  The hazard: inside group_values wave 0 reads sh.gdiag in its 6 x 6 Cholesky
// AFTER the function's last barrier, so fold f + 1 may be staged only behind a barrier that follows fold f's return --
// the barrier that ends a step anyway (the next group_values writes sh.idx, which that Cholesky reads too) ends a
// fold-step here.  The staged words are published by group_values' own first barrier, before anyone reads them.
__device__ inline GroupArgs fold_args(const GroupArgs& a, int f) {
  GroupArgs b = a;
  b.G += (int64_t)f * a.p * a.ldg;
  b.H += (int64_t)f * a.p * a.ldh;
  b.g += (int64_t)f * a.p;
  b.h += (int64_t)f * a.p;
  b.inv_yy = a.inv_yy_rep[f];
  return b;
}

// h and the pivot scale of one fold into sh; the caller's last barrier is behind every read of them
__device__ inline void stage_fold(GrpShared& sh, const GroupArgs& a, int tid) {
  if (tid < a.p) {
    sh.h[tid] = a.h[tid];
    sh.gdiag[tid] = a.G[(int64_t)tid * a.ldg + tid];
  }
}

// a.part [units][g + 1], bm [units][g + 1][2] as groups_best_kernel's; a.info [F]
__global__ __launch_bounds__(NT) void groups_cv_best_kernel(GroupArgs a, int F, uint64_t s0, uint64_t s1, GroupIds ids,
                                                            uint32_t* __restrict__ bm) {
  __shared__ GrpShared sh;
  __shared__ GrpBestShared sb;
  const int tid = threadIdx.x;
  const int ng = a.ng, gl = a.gl, gh = a.gh;
  const bool live = tid < (1 << gl);           // wave 0 only (gl <= 6)
  if (tid < GG) sb.gid[tid] = ids.id[tid];
  if (live) {
    for (int j = 0; j < GBS; ++j) {            // the lane's own slots: nobody else reads or writes them
      sb.v[j * 64 + tid] = -__builtin_huge_val();
      sb.h[j * 64 + tid] = 0u;
    }
  }
  load_shared<false>(sh, a, tid);              // (ends with a barrier: gid; h and gdiag are restaged per fold)
  uint32_t bad_folds = 0u;                     // bit f: a pivot of fold f failed in a subset this thread saw
  for (uint64_t s = s0; s < s1; ++s) {
    const uint64_t hi = (uint64_t)blockIdx.x * a.per + s;
    double v = 0.0;
    bool bad_any = false;                      // this subset's own pivots, over the folds
#pragma unroll 1
    for (int f = 0; f < F; ++f) {
      const GroupArgs af = fold_args(a, f);
      stage_fold(sh, af, tid);
      bool bad = false;
      const double vf = group_values<false>(sh, af, hi, tid, bad);
      v = f == 0 ? vf : v + vf;
      bad_any |= bad;
      bad_folds |= bad ? (1u << f) : 0u;
      __syncthreads();
    }
    // the lane's own slots, written behind the step's last barrier: nobody else touches them (groups_best_kernel)
    if (live && !bad_any) {
      const int e = __popcll(s) * 64 + tid;    // popc(s) < GBS: launch_groups_cv_best
      if (v > sb.v[e]) {
        sb.v[e] = v;
        sb.h[e] = (uint32_t)hi;                // gh <= 31
      }
    }
  }
  if (tid < 64) {
    double* rv = a.part + (int64_t)blockIdx.x * (ng + 1);
    uint32_t* rm = bm + (int64_t)blockIdx.x * (ng + 1) * 2;
    const int ncls = __popcll(a.per - 1) + 1;
    const int k0 = __popc(blockIdx.x), k1 = min(ng, k0 + ncls - 1 + gl);
    const int base = k0 + __popc(tid);         // |S| of this lane's class 0
    uint32_t low = 0u;                         // the lane's low groups in the caller's numbering
    for (int r = 0; r < gl; ++r)
      if ((tid >> r) & 1) low |= 1u << sb.gid[r];
    for (int k = k0; k <= k1; ++k) {
      const int j = k - base;
      double v = -__builtin_huge_val();
      uint32_t mask = 0u;
      if (live && j >= 0 && j < ncls) {
        v = sb.v[j * 64 + tid];
        const uint32_t h = sb.h[j * 64 + tid];
        mask = low;
        for (int r = 0; r < gh; ++r)
          if ((h >> r) & 1u) mask |= 1u << sb.gid[gl + r];
      }
      wave_best(v, mask);                      // over caller masks, as in groups_best_kernel
      if (tid == 0 && v > -__builtin_huge_val()) {
        if (rm[2 * k + 1] != 0u) best_merge(v, mask, rv[k], rm[2 * k]);
        rv[k] = v;
        rm[2 * k] = mask;
        rm[2 * k + 1] = 1u;
      }
    }
  }
  for (int f = 0; f < F; ++f)
    if (__any((bad_folds >> f) & 1u) && (tid & 63) == 0) atomicOr(a.info + f, 1);
}

// test hook and the winners' per-fold values: vals[i] = u_cv(masks[i]), vfold[i][f] = u_f(masks[i]) (vfold may be null),
// masks in the layout's numbering, by the very fold-step of groups_cv_best_kernel
__global__ __launch_bounds__(NT) void groups_cv_debug_kernel(GroupArgs a, int F, const uint64_t* __restrict__ masks,
                                                             int64_t n, double* __restrict__ vals,
                                                             double* __restrict__ vfold) {
  __shared__ GrpShared sh;
  const int tid = threadIdx.x;
  load_shared<false>(sh, a, tid);
  uint32_t bad_folds = 0u;
  const uint64_t low = (1ull << a.gl) - 1ull;
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint64_t m = masks[i];
    const bool mine = (uint64_t)tid == (m & low);
    double v = 0.0;
#pragma unroll 1
    for (int f = 0; f < F; ++f) {
      const GroupArgs af = fold_args(a, f);
      stage_fold(sh, af, tid);
      bool bad = false;
      const double vf = group_values<false>(sh, af, m >> a.gl, tid, bad);
      v = f == 0 ? vf : v + vf;
      bad_folds |= bad ? (1u << f) : 0u;
      if (mine && vfold) vfold[i * F + f] = vf;
      __syncthreads();
    }
    if (mine) vals[i] = v;
  }
  for (int f = 0; f < F; ++f)
    if (__any((bad_folds >> f) & 1u) && (tid & 63) == 0) atomicOr(a.info + f, 1);
}

// ---- the T best group subsets of every size (lsspa_groups_top) ----
// groups_best_kernel's sibling, one problem only: the same workgroup, units, steps and launches, load_shared<false> and
// group_values<false>, the same candidates (the subset's own pivots passed, its value is above -inf, so never NaN) and
// the same total order -- the larger value first, on equal values the numerically smaller mask in the CALLER's
// numbering.  What is kept per size k is not one winner but the T best, 1 <= T <= GROUPS_TOP_MAX.  Masks are unique, so
// the order is strict and the T best of any collection of subsets are one definite list: the result depends neither on
// the cut into units and launches nor on the order of the inserts.
//   Lists: |S| = popc(unit) + popc(s) + popc(lane), so a unit meets at most GTS = (GBS - 1) + GQ + 1 = 25 sizes,
// popc(unit) + j with j = popc(s) + popc(lane).  Per such j it keeps a sorted list of up to T (value, caller mask) and a
// count in LDS, k_subsets.hip's subsets_top_kernel's lists at a fixed row stride of GROUPS_TOP_MAX: 4.9 KB beside
// GrpShared, against the sibling's 14.6 KB.  The lists hold caller masks, for the threshold compare and the rank go by
// the caller's order: a lane's low part is fixed and translated once, the high part of hi is the same for the whole
// workgroup and translated once per step from the kernel's own arguments (GroupIds), on the scalar unit.  A launch loads
// the unit's lists from its rows of the table and stores them back at its end (one workgroup owns a row, launches are
// ordered by the stream: plain loads and stores); the counts are cleared before the first launch, the entries need
// not be.
//   Fast path and insert are subsets_top_kernel's: a live lane compares its value with its list's last entry, one ballot
// says whether anything is to be inserted, and the insert is a wave-wide rank-and-shift with lane t < T holding entry t.
// The one difference: four waves run the step, only wave 0 holds values.  The lists are wave 0's alone -- loaded before
// load_shared's barrier, read and written between the last barrier of group_values and the barrier that ends the step,
// stored after the last step's -- and the insert loop, which only wave 0 executes, contains no workgroup barrier.  What
// orders its LDS writes against the reads of the next round is the wave itself: the 64 lanes are one instruction stream,
// the LDS executes one wave's instructions in the order of their issue, and wave_lds_fence (a release/acquire fence of
// wavefront scope, no instruction of its own) keeps the compiler from moving a read of the lists over a write of them
// or from keeping an entry in a register across the round.
constexpr int GTS = (GBS - 1) + GQ + 1;        // sizes a unit meets at most
constexpr int GTM = GROUPS_TOP_MAX;            // row stride of the lists in LDS

struct GrpTopShared {
  double v[GTS * GTM];     // [size j][rank]: the unit's best values of size popc(unit) + j, best first
  uint32_t m[GTS * GTM];   // their caller masks
  int c[GTS];              // valid entries of a list
  int gid[GG];
};

// does (v, m) come before (ov, om) in the total order? (k_subsets.hip, top_before)
__device__ inline bool top_before(double v, uint32_t m, double ov, uint32_t om) { return v > ov || (v == ov && m < om); }

// orders one wave's LDS accesses in program order (the header of this section)
__device__ inline void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a.part [units][g + 1][T] (values), tm [units][g + 1][T] (caller masks), tc [units][g + 1] (counts): unit u's T best of
// every size so far, best first
__global__ __launch_bounds__(NT) void groups_top_kernel(GroupArgs a, uint64_t s0, uint64_t s1, GroupIds ids, int T,
                                                        uint32_t* __restrict__ tm, int32_t* __restrict__ tc) {
  __shared__ GrpShared sh;
  __shared__ GrpTopShared st;
  const int tid = threadIdx.x;
  const int ng = a.ng, gl = a.gl;
  const bool live = tid < (1 << gl);           // wave 0 only (gl <= 6)
  // the sizes this unit can hold: k0 + j, j < ns (popc(s) + popc(lane) with s < per, lane < 2^gl, and no more than ng)
  const int k0 = __popc(blockIdx.x);
  const int ns = min(ng - k0, __popcll(a.per - 1) + gl) + 1;       // <= GTS: launch_groups_top
  double* gv = a.part + ((int64_t)blockIdx.x * (ng + 1) + k0) * T;
  uint32_t* gm = tm + ((int64_t)blockIdx.x * (ng + 1) + k0) * T;
  int32_t* gc = tc + (int64_t)blockIdx.x * (ng + 1) + k0;
  if (tid < 64) {
    for (int e = tid; e < ns * T; e += 64) {
      const int j = e / T, r = e - j * T;
      if (r < gc[j]) {
        st.v[j * GTM + r] = gv[e];
        st.m[j * GTM + r] = gm[e];
      }
    }
    if (tid < ns) st.c[tid] = gc[tid];
  }
  if (tid < GG) st.gid[tid] = ids.id[tid];
  load_shared<false>(sh, a, tid);              // (ends with a barrier: the lists, gid)
  uint32_t low = 0u;                           // the lane's low groups in the caller's numbering
  for (int r = 0; r < gl; ++r)
    if ((tid >> r) & 1) low |= 1u << st.gid[r];
  const int jl = live ? __popc(tid) : 0;
  bool any_bad = false;
  for (uint64_t s = s0; s < s1; ++s) {
    const uint64_t hi = (uint64_t)blockIdx.x * a.per + s;
    bool bad = false;                          // this subset's own pivots, as in groups_best_kernel
    const double v = group_values<false>(sh, a, hi, tid, bad);
    any_bad |= bad;
    if (tid < 64) {                            // wave 0: no workgroup barrier in here
      // the high groups of hi in the caller's numbering: the same for every lane (gh <= 31)
      uint32_t hm = 0u;
      for (uint32_t b = (uint32_t)hi; b != 0u; b &= b - 1u) hm |= 1u << ids.id[gl + __ffs((int)b) - 1];
      const uint32_t m = hm | low;
      const int j = __popcll(s) + jl;          // < ns for every live lane
      // a candidate that belongs into its size's list as it is now: the list is not full, or its last entry comes later
      auto wanted = [&]() {
        return st.c[j] < T || top_before(v, m, st.v[j * GTM + T - 1], st.m[j * GTM + T - 1]);
      };
      bool want = live && !bad && v > -__builtin_huge_val() && wanted();
      for (uint64_t todo = __ballot(want); todo != 0ull; todo = __ballot(want)) {
        const int src = __ffsll((unsigned long long)todo) - 1;
        const double nv = __shfl(v, src, 64);
        const uint32_t nm = (uint32_t)__shfl((int)m, src, 64);
        const int nj = __shfl(j, src, 64);
        double* rv = st.v + nj * GTM;
        uint32_t* rm = st.m + nj * GTM;
        const int c = st.c[nj];
        const bool have = tid < c;             // c <= T <= 16: lane t holds entry t
        const double ev = have ? rv[tid] : 0.0;
        const uint32_t em = have ? rm[tid] : 0u;
        const int rank = __popcll(__ballot(have && top_before(ev, em, nv, nm)));
        const double pv = __shfl_up(ev, 1, 64);
        const uint32_t pm = (uint32_t)__shfl_up((int)em, 1, 64);
        const int nc = min(c + 1, T);
        wave_lds_fence();                      // every lane has read its entry and the count
        if (tid >= rank && tid < nc) {         // a lane writes the entry it read: no other lane's
          rv[tid] = tid == rank ? nv : pv;
          rm[tid] = tid == rank ? nm : pm;
        }
        if (tid == 0) st.c[nj] = nc;
        wave_lds_fence();                      // the list as it now is, for every lane
        if (tid == src) want = false;
        want = want && wanted();
      }
    }
    __syncthreads();
  }
  if (tid < 64) {
    for (int e = tid; e < ns * T; e += 64) {
      const int j = e / T, r = e - j * T;
      if (r < st.c[j]) {
        gv[e] = st.v[j * GTM + r];
        gm[e] = st.m[j * GTM + r];
      }
    }
    if (tid < ns) gc[tid] = st.c[tid];
  }
  if (__any(any_bad) && (tid & 63) == 0) atomicOr(a.info, 1);
}

// ---- the T best group subsets of every size by the K-fold cross-validated value (lsspa_cv_groups_top) ----
// groups_cv_best_kernel's fold-step with groups_top_kernel's lists; neither sibling changes.  The same workgroup, units,
// per, steps and launches as groups_cv_best_kernel; load_shared<false> once; per step and per fold f = 0 .. F-1, in this
// order: fold_args, stage_fold, group_values<false> on fold f's addresses, u = f == 0 ? u_f : u + u_f, the barrier that
// ends the fold-step.  So every u_f has the bits groups_cv_debug_kernel gives and the sum is formed in fold order.  A
// subset is a candidate if its own pivots passed in EVERY fold and its sum is above -inf (so never NaN); a failed pivot
// raises the info word of the fold it failed in, as in groups_cv_best_kernel.  Lists, table, order (top_before over
// CALLER masks: the lane's low part translated once, the high part once per step from GroupIds -- it is the same for all
// folds of the step), fast path and wave-wide rank-and-shift insert are groups_top_kernel's, unchanged in logic.
//   Hazards:
//   - the lists (st.v, st.m, st.c) are wave 0's alone: loaded by wave 0 before load_shared's barrier, read and written by
//     wave 0 in the insert, stored by wave 0 after the last step.  The insert loop contains no workgroup barrier and is
//     executed by wave 0 only; wave_lds_fence orders its rounds (the header of groups_top_kernel);
//   - the insert runs once per step, after the last fold's value is known, BEHIND the last fold-step's closing barrier
//     and before the next step's first group_values -- where groups_cv_best_kernel updates its slots.  The next barrier
//     all four waves reach is the first one inside that group_values (or, after the last step, none: the store of the
//     lists is wave 0's own, in program order behind the insert).  Meanwhile the other three waves may already stage
//     the next step's fold 0 into sh.h / sh.gdiag and write sh.idx: the insert reads and writes nothing of GrpShared --
//     its operands are registers, the kernel's arguments and the lists -- and wave 0's own reads of sh.gdiag, sh.idx,
//     sh.M and sh.Z in the last fold's 6 x 6 Cholesky are in front of the closing barrier.  The alternative, the insert
//     in front of that barrier (groups_top_kernel's place), needs a test of f inside the fold loop and keeps three waves
//     idle at the barrier for the length of the insert instead of letting them issue the next fold's loads;
//   - stage_fold for fold f + 1 comes only behind the barrier that follows fold f's return (the 6 x 6 Cholesky hazard
//     described above groups_cv_best_kernel): the structure of that kernel's fold loop is kept;
//   - LDS is GrpShared + GrpTopShared, static, for every F and T: 4.9 KB beside GrpShared against the best-kernel's
//     14.6 KB (groups_cv_top_lds_bytes), three workgroups a CU where groups_cv_best_kernel has two.
// a.part [units][g + 1][T], tm [units][g + 1][T], tc [units][g + 1] as groups_top_kernel's; a.info [F]
__global__ __launch_bounds__(NT) void groups_cv_top_kernel(GroupArgs a, int F, uint64_t s0, uint64_t s1, GroupIds ids,
                                                           int T, uint32_t* __restrict__ tm, int32_t* __restrict__ tc) {
  __shared__ GrpShared sh;
  __shared__ GrpTopShared st;
  const int tid = threadIdx.x;
  const int ng = a.ng, gl = a.gl;
  const bool live = tid < (1 << gl);           // wave 0 only (gl <= 6)
  // the sizes this unit can hold: k0 + j, j < ns (popc(s) + popc(lane) with s < per, lane < 2^gl, and no more than ng)
  const int k0 = __popc(blockIdx.x);
  const int ns = min(ng - k0, __popcll(a.per - 1) + gl) + 1;       // <= GTS: launch_groups_cv_top
  double* gv = a.part + ((int64_t)blockIdx.x * (ng + 1) + k0) * T;
  uint32_t* gm = tm + ((int64_t)blockIdx.x * (ng + 1) + k0) * T;
  int32_t* gc = tc + (int64_t)blockIdx.x * (ng + 1) + k0;
  if (tid < 64) {
    for (int e = tid; e < ns * T; e += 64) {
      const int j = e / T, r = e - j * T;
      if (r < gc[j]) {
        st.v[j * GTM + r] = gv[e];
        st.m[j * GTM + r] = gm[e];
      }
    }
    if (tid < ns) st.c[tid] = gc[tid];
  }
  if (tid < GG) st.gid[tid] = ids.id[tid];
  load_shared<false>(sh, a, tid);              // (ends with a barrier: the lists, gid; h and gdiag are restaged per fold)
  uint32_t low = 0u;                           // the lane's low groups in the caller's numbering
  for (int r = 0; r < gl; ++r)
    if ((tid >> r) & 1) low |= 1u << st.gid[r];
  const int jl = live ? __popc(tid) : 0;
  uint32_t bad_folds = 0u;                     // bit f: a pivot of fold f failed in a subset this thread saw
  for (uint64_t s = s0; s < s1; ++s) {
    const uint64_t hi = (uint64_t)blockIdx.x * a.per + s;
    double v = 0.0;
    bool bad_any = false;                      // this subset's own pivots, over the folds
#pragma unroll 1
    for (int f = 0; f < F; ++f) {
      const GroupArgs af = fold_args(a, f);
      stage_fold(sh, af, tid);
      bool bad = false;
      const double vf = group_values<false>(sh, af, hi, tid, bad);
      v = f == 0 ? vf : v + vf;
      bad_any |= bad;
      bad_folds |= bad ? (1u << f) : 0u;
      __syncthreads();
    }
    // behind the step's last barrier, in front of the next group_values' first: the lists are wave 0's (the header)
    if (tid < 64) {                            // wave 0: no workgroup barrier in here
      // the high groups of hi in the caller's numbering: the same for every lane and every fold (gh <= 31)
      uint32_t hm = 0u;
      for (uint32_t b = (uint32_t)hi; b != 0u; b &= b - 1u) hm |= 1u << ids.id[gl + __ffs((int)b) - 1];
      const uint32_t m = hm | low;
      const int j = __popcll(s) + jl;          // < ns for every live lane
      // a candidate that belongs into its size's list as it is now: the list is not full, or its last entry comes later
      auto wanted = [&]() {
        return st.c[j] < T || top_before(v, m, st.v[j * GTM + T - 1], st.m[j * GTM + T - 1]);
      };
      bool want = live && !bad_any && v > -__builtin_huge_val() && wanted();
      for (uint64_t todo = __ballot(want); todo != 0ull; todo = __ballot(want)) {
        const int src = __ffsll((unsigned long long)todo) - 1;
        const double nv = __shfl(v, src, 64);
        const uint32_t nm = (uint32_t)__shfl((int)m, src, 64);
        const int nj = __shfl(j, src, 64);
        double* rv = st.v + nj * GTM;
        uint32_t* rm = st.m + nj * GTM;
        const int c = st.c[nj];
        const bool have = tid < c;             // c <= T <= 16: lane t holds entry t
        const double ev = have ? rv[tid] : 0.0;
        const uint32_t em = have ? rm[tid] : 0u;
        const int rank = __popcll(__ballot(have && top_before(ev, em, nv, nm)));
        const double pv = __shfl_up(ev, 1, 64);
        const uint32_t pm = (uint32_t)__shfl_up((int)em, 1, 64);
        const int nc = min(c + 1, T);
        wave_lds_fence();                      // every lane has read its entry and the count
        if (tid >= rank && tid < nc) {         // a lane writes the entry it read: no other lane's
          rv[tid] = tid == rank ? nv : pv;
          rm[tid] = tid == rank ? nm : pm;
        }
        if (tid == 0) st.c[nj] = nc;
        wave_lds_fence();                      // the list as it now is, for every lane
        if (tid == src) want = false;
        want = want && wanted();
      }
    }
  }
  if (tid < 64) {                              // wave 0, behind its own last insert
    for (int e = tid; e < ns * T; e += 64) {
      const int j = e / T, r = e - j * T;
      if (r < st.c[j]) {
        gv[e] = st.v[j * GTM + r];
        gm[e] = st.m[j * GTM + r];
      }
    }
    if (tid < ns) gc[tid] = st.c[tid];
  }
  for (int f = 0; f < F; ++f)
    if (__any((bad_folds >> f) & 1u) && (tid & 63) == 0) atomicOr(a.info + f, 1);
}

// masks in the layout's own numbering: bits 0 .. gl-1 the low groups, then the high ones
__global__ __launch_bounds__(NT) void groups_debug_kernel(GroupArgs a, const uint64_t* __restrict__ masks, int64_t n,
                                                          double* __restrict__ vals) {
  __shared__ GrpShared sh;
  const int tid = threadIdx.x;
  load_shared<false>(sh, a, tid);
  bool bad = false;
  const uint64_t low = (1ull << a.gl) - 1ull;
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint64_t m = masks[i];
    const double v = group_values<false>(sh, a, m >> a.gl, tid, bad);
    if ((uint64_t)tid == (m & low)) vals[i] = v;
    __syncthreads();
  }
  if (__any(bad) && (tid & 63) == 0) atomicOr(a.info, 1);
}

bool args_ok(const GroupArgs& a) {
  return a.p >= 1 && a.p <= GP && a.ng >= 1 && a.ng <= GG && a.gl >= 0 && a.gl <= GQ && a.gl + a.gh == a.ng &&
         a.ql >= a.gl && a.ql <= GQ && a.nb >= 0 && a.nb + a.ql <= a.p && a.G && a.g && a.H && a.h && a.w && a.tab &&
         a.info && a.ldg >= a.p && a.ldh >= a.p;
}

}  // namespace

const char* groups_layout(const int32_t* labels, int p, int g, GroupLayout& L) {
  if (!labels) return "labels is NULL";
  if (g < 1) return "grouped attribution needs at least one group";
  if (g > GG) return "grouped attribution takes at most 32 groups";
  if (p < 1 || p > GP) return "grouped attribution takes at most 64 columns";
  int size[GG] = {0};
  L = GroupLayout{};
  for (int j = 0; j < p; ++j) {
    if (labels[j] < -1 || labels[j] >= g) return "a label lies outside -1 .. g-1";
    if (labels[j] >= 0) ++size[labels[j]];
  }
  for (int k = 0; k < g; ++k)
    if (size[k] == 0) return "a group of 0 .. g-1 has no column";
  // low groups: the smallest first (ties by number) while their columns fit the register-resident Cholesky
  int order[GG];
  std::iota(order, order + g, 0);
  std::stable_sort(order, order + g, [&](int x, int y) { return size[x] < size[y]; });
  bool low[GG] = {false};
  L.p = p;
  L.ng = g;
  for (int r = 0; r < g && L.ql + size[order[r]] <= GQ; ++r) {
    low[order[r]] = true;
    L.gid[L.gl++] = order[r];
    L.ql += size[order[r]];
  }
  L.gh = g - L.gl;
  for (int k = 0, j = 0; k < g; ++k)
    if (!low[k]) L.gid[L.gl + j++] = k;
  int32_t* cols = L.tab + GROUPS_TAB_COLS;
  int32_t* colgrp = L.tab + GROUPS_TAB_COLGRP;
  int32_t* colin = L.tab + GROUPS_TAB_COLIN;
  int c = 0;
  for (int j = 0; j < p; ++j)
    if (labels[j] < 0) {
      colgrp[c] = -1;
      cols[c++] = j;
    }
  L.nb = c;
  for (int r = L.gl; r < g; ++r) {
    int n = 0;
    for (int j = 0; j < p; ++j)
      if (labels[j] == L.gid[r]) {
        colgrp[c] = r - L.gl;
        colin[c] = n++;
        cols[c++] = j;
      }
    L.tab[GROUPS_TAB_HSIZE + r - L.gl] = n;
  }
  for (int r = 0, t = 0; r < L.gl; ++r)
    for (int j = 0; j < p; ++j)
      if (labels[j] == L.gid[r]) {
        colgrp[c] = -1;
        L.tab[GROUPS_TAB_LGRP + t++] = r;
        cols[c++] = j;
      }
  return nullptr;
}

hipError_t launch_groups_enum(const GroupArgs& a, uint64_t units, uint64_t s0, uint64_t s1, bool inter,
                              hipStream_t st, int reps) {
  if (!args_ok(a) || !a.part || units < 1 || s1 <= s0 || s1 > a.per) return hipErrorInvalidValue;
  // replicates: with inv_yy_rep, at most 2^20 workgroups a launch (the caller vouches for `reps` problems, tables, info
  // words behind the first); one problem: no inv_yy_rep
  if (reps < 1 || reps > 65535 || (a.inv_yy_rep ? units * (uint64_t)reps > (1ull << 20) : reps != 1))
    return hipErrorInvalidValue;
  // every high subset index of the launch must exist: unit u covers [u per, (u + 1) per) of 2^gh
  if (units * a.per != (1ull << a.gh) || units > (1ull << 31)) return hipErrorInvalidValue;
  if (inter) {
    if (a.gh > GHI) return hipErrorInvalidValue;   // the kernel's pair masks (no layout of <= 64 columns has more)
    if (a.inv_yy_rep)
      hipLaunchKernelGGL((groups_enum_kernel<true, true>), dim3((unsigned)units, (unsigned)reps), dim3(NT), 0, st, a, s0,
                         s1);
    else
      hipLaunchKernelGGL(groups_enum_kernel<true>, dim3((unsigned)units), dim3(NT), 0, st, a, s0, s1);
  } else if (a.inv_yy_rep) {
    hipLaunchKernelGGL((groups_enum_kernel<false, true>), dim3((unsigned)units, (unsigned)reps), dim3(NT), 0, st, a, s0,
                       s1);
  } else {
    hipLaunchKernelGGL(groups_enum_kernel<false>, dim3((unsigned)units), dim3(NT), 0, st, a, s0, s1);
  }
  return hipGetLastError();
}

hipError_t launch_groups_owen(const GroupArgs& a, uint64_t units, uint64_t s0, uint64_t s1, hipStream_t st) {
  if (!args_ok(a) || !a.part || units < 1 || s1 <= s0 || s1 > a.per) return hipErrorInvalidValue;
  if (a.inv_yy_rep) return hipErrorInvalidValue;     // no replicates: one problem
  // the kernel's mask of the inner players among the high ones is 32 bits wide (no layout of <= 64 columns has gh = 32)
  if (a.gh > GHI) return hipErrorInvalidValue;
  if (units * a.per != (1ull << a.gh) || units > (1ull << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL((groups_enum_kernel<false, false, true>), dim3((unsigned)units), dim3(NT), 0, st, a, s0, s1);
  return hipGetLastError();
}

hipError_t launch_groups_best(const GroupArgs& a, const int* gid, uint64_t units, uint64_t s0, uint64_t s1, uint32_t* bm,
                              hipStream_t st, int reps) {
  if (!args_ok(a) || !a.part || !bm || !gid || units < 1 || s1 <= s0 || s1 > a.per) return hipErrorInvalidValue;
  // replicates: launch_groups_enum's terms (the caller vouches for `reps` problems, rows of both tables and info words)
  if (reps < 1 || reps > 65535 || (a.inv_yy_rep ? units * (uint64_t)reps > (1ull << 20) : reps != 1))
    return hipErrorInvalidValue;
  if (a.gh > GHI) return hipErrorInvalidValue;       // hi is kept in 32 bits (no layout of <= 64 columns has gh = 32)
  if (units * a.per != (1ull << a.gh) || units > (1ull << 31)) return hipErrorInvalidValue;
  // the size classes of a unit are popc(s), s < per: per a power of two (it is: units per = 2^gh) of at most GBS - 1 bits
  if (a.per > (1ull << (GBS - 1))) return hipErrorInvalidValue;
  GroupIds ids{};
  uint32_t seen = 0u;
  for (int r = 0; r < a.ng; ++r) {                   // a permutation of 0 .. ng-1: the kernel shifts by them
    if (gid[r] < 0 || gid[r] >= a.ng || ((seen >> gid[r]) & 1u)) return hipErrorInvalidValue;
    seen |= 1u << gid[r];
    ids.id[r] = (uint8_t)gid[r];
  }
  if (a.inv_yy_rep)
    hipLaunchKernelGGL(groups_best_kernel<true>, dim3((unsigned)units, (unsigned)reps), dim3(NT), 0, st, a, s0, s1, ids,
                       bm);
  else
    hipLaunchKernelGGL(groups_best_kernel<false>, dim3((unsigned)units), dim3(NT), 0, st, a, s0, s1, ids, bm);
  return hipGetLastError();
}

hipError_t launch_groups_top(const GroupArgs& a, const int* gid, uint64_t units, uint64_t s0, uint64_t s1, int T,
                             uint32_t* tm, int32_t* tc, hipStream_t st) {
  if (!args_ok(a) || !a.part || !tm || !tc || !gid || units < 1 || s1 <= s0 || s1 > a.per) return hipErrorInvalidValue;
  if (T < 1 || T > GROUPS_TOP_MAX) return hipErrorInvalidValue;
  if (a.inv_yy_rep) return hipErrorInvalidValue;     // no replicates: one problem
  if (a.gh > GHI) return hipErrorInvalidValue;       // hi is kept in 32 bits (no layout of <= 64 columns has gh = 32)
  if (units * a.per != (1ull << a.gh) || units > (1ull << 31)) return hipErrorInvalidValue;
  // the sizes of a unit are popc(s) + popc(lane), s < per: per a power of two of at most GBS - 1 bits, GTS lists
  if (a.per > (1ull << (GBS - 1))) return hipErrorInvalidValue;
  GroupIds ids{};
  uint32_t seen = 0u;
  for (int r = 0; r < a.ng; ++r) {                   // a permutation of 0 .. ng-1: the kernel shifts by them
    if (gid[r] < 0 || gid[r] >= a.ng || ((seen >> gid[r]) & 1u)) return hipErrorInvalidValue;
    seen |= 1u << gid[r];
    ids.id[r] = (uint8_t)gid[r];
  }
  hipLaunchKernelGGL(groups_top_kernel, dim3((unsigned)units), dim3(NT), 0, st, a, s0, s1, ids, T, tm, tc);
  return hipGetLastError();
}

// the two __shared__ objects both kernels declare, each at the 16-byte alignment the compiler gives them (its
// resource report says 58352 for both)
static constexpr size_t lds16(size_t n) { return (n + 15) / 16 * 16; }
size_t groups_best_lds_bytes() { return lds16(sizeof(GrpShared)) + lds16(sizeof(GrpBestShared)); }
size_t groups_cv_lds_bytes() { return lds16(sizeof(GrpShared)) + lds16(sizeof(GrpBestShared)); }

hipError_t launch_groups_cv_best(const GroupArgs& a, int folds, const int* gid, uint64_t units, uint64_t s0, uint64_t s1,
                                 uint32_t* bm, hipStream_t st) {
  if (!args_ok(a) || !a.part || !bm || !gid || units < 1 || s1 <= s0 || s1 > a.per) return hipErrorInvalidValue;
  // the caller vouches for `folds` problems, denominators (inv_yy_rep) and info words behind the first
  if (!a.inv_yy_rep || folds < 2 || folds > CV_MAX_FOLDS) return hipErrorInvalidValue;
  if (a.gh > GHI) return hipErrorInvalidValue;       // hi is kept in 32 bits (no layout of <= 64 columns has gh = 32)
  if (units * a.per != (1ull << a.gh) || units > (1ull << 31)) return hipErrorInvalidValue;
  if (a.per > (1ull << (GBS - 1))) return hipErrorInvalidValue;
  GroupIds ids{};
  uint32_t seen = 0u;
  for (int r = 0; r < a.ng; ++r) {                   // a permutation of 0 .. ng-1: the kernel shifts by them
    if (gid[r] < 0 || gid[r] >= a.ng || ((seen >> gid[r]) & 1u)) return hipErrorInvalidValue;
    seen |= 1u << gid[r];
    ids.id[r] = (uint8_t)gid[r];
  }
  hipLaunchKernelGGL(groups_cv_best_kernel, dim3((unsigned)units), dim3(NT), 0, st, a, folds, s0, s1, ids, bm);
  return hipGetLastError();
}

// groups_cv_top_kernel's two: the compiler lays the lists first, padded to 16 bytes, and GrpShared (a multiple of 8)
// behind them; its resource report says 48664, for this kernel and for groups_top_kernel
size_t groups_cv_top_lds_bytes() { return lds16(sizeof(GrpTopShared)) + sizeof(GrpShared); }

hipError_t launch_groups_cv_top(const GroupArgs& a, int folds, const int* gid, uint64_t units, uint64_t s0, uint64_t s1,
                                int T, uint32_t* tm, int32_t* tc, hipStream_t st) {
  if (!args_ok(a) || !a.part || !tm || !tc || !gid || units < 1 || s1 <= s0 || s1 > a.per) return hipErrorInvalidValue;
  if (T < 1 || T > GROUPS_TOP_MAX) return hipErrorInvalidValue;
  // the caller vouches for `folds` problems, denominators (inv_yy_rep) and info words behind the first
  if (!a.inv_yy_rep || folds < 2 || folds > CV_MAX_FOLDS) return hipErrorInvalidValue;
  if (a.gh > GHI) return hipErrorInvalidValue;       // hi is kept in 32 bits (no layout of <= 64 columns has gh = 32)
  if (units * a.per != (1ull << a.gh) || units > (1ull << 31)) return hipErrorInvalidValue;
  // the sizes of a unit are popc(s) + popc(lane), s < per: per a power of two of at most GBS - 1 bits, GTS lists
  if (a.per > (1ull << (GBS - 1))) return hipErrorInvalidValue;
  if (__builtin_popcountll(a.per - 1) + a.gl + 1 > GTS) return hipErrorInvalidValue;
  GroupIds ids{};
  uint32_t seen = 0u;
  for (int r = 0; r < a.ng; ++r) {                   // a permutation of 0 .. ng-1: the kernel shifts by them
    if (gid[r] < 0 || gid[r] >= a.ng || ((seen >> gid[r]) & 1u)) return hipErrorInvalidValue;
    seen |= 1u << gid[r];
    ids.id[r] = (uint8_t)gid[r];
  }
  hipLaunchKernelGGL(groups_cv_top_kernel, dim3((unsigned)units), dim3(NT), 0, st, a, folds, s0, s1, ids, T, tm, tc);
  return hipGetLastError();
}

hipError_t launch_groups_cv_debug(const GroupArgs& a, int folds, const uint64_t* masks, int64_t n, double* vals,
                                  double* vfold, hipStream_t st) {
  if (!args_ok(a) || !masks || !vals || n < 1) return hipErrorInvalidValue;
  if (!a.inv_yy_rep || folds < 2 || folds > CV_MAX_FOLDS) return hipErrorInvalidValue;
  const int64_t grid = n < 4096 ? n : 4096;
  hipLaunchKernelGGL(groups_cv_debug_kernel, dim3((unsigned)grid), dim3(NT), 0, st, a, folds, masks, n, vals, vfold);
  return hipGetLastError();
}

hipError_t launch_groups_debug(const GroupArgs& a, const uint64_t* masks, int64_t n, double* vals, hipStream_t st) {
  if (!args_ok(a) || !masks || !vals || n < 1) return hipErrorInvalidValue;
  const int64_t grid = n < 4096 ? n : 4096;
  hipLaunchKernelGGL(groups_debug_kernel, dim3((unsigned)grid), dim3(NT), 0, st, a, masks, n, vals);
  return hipGetLastError();
}

}  // namespace lsspa
