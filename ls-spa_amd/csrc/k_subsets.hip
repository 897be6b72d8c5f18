// Exact Shapley attribution by subset enumeration (p <= 32): v(K) of all 2^p feature subsets, never stored, folded
// into the Shapley sum as it is computed.  fp64 throughout, whatever the per-ordering precision says.
//
// With G, g (training side) and H, h (test side) of the reduced problem, for a subset K
//   theta_K = G_KK^-1 g_K,   v(K) = (2 theta_K^T h_K - theta_K^T H_KK theta_K) / ||y_test||^2,   v({}) = 0,
// the out-of-sample R^2 of the prefix set K in square_shapley (the reference's ls_spa/ls_spa.py:275-285), and
//   phi_j = sum_{S not containing j} w(|S|) (v(S + j) - v(S)),   w(k) = k! (p - 1 - k)! / p!.
//
// Decomposition ("Exact attribution by subset enumeration"): the features split into q = min(p, 6) LOW ones
// (features 0 .. q-1) and p - q HIGH ones.  One wave owns one high subset Hs at a time:
//   1. it sweeps (Gauss-Jordan in Goodnight's form) the pivots of Hs out of the compacted augmented matrix
//      [G g; g^T 0] over Hs + low features, which leaves A^-1 [B g] in the Hs rows (A = G_HsHs, B = G_Hs,low) and the
//      Schur complement S = G_LL - B^T A^-1 B, g~ = g_L - B^T A^-1 g_Hs in the low block;
//   2. theta over Hs + T is e0 + E theta_T with e0 = [A^-1 g_Hs; 0], E = [-A^-1 B; I]: the test side reduces to the
//      (q+1) x (q+1) matrix Z = X^T H X and z = X^T h of X = [e0 E], whence f0, r and W of
//        v(Hs + T) = (f0 + 2 theta_T^T r_T - theta_T^T W_TT theta_T) / ||y||^2,   theta_T = S_TT^-1 g~_T;
//   3. lane T (one lane per low subset, 2^6 = 64) masks rows and columns of S outside T to the identity and runs the
//      same fixed 6 x 6 Cholesky, solve and quadratic form as every other lane: no divergence on |T|.
// The Shapley sum: with a(K) = w(|K| - 1) v(K) (|K| >= 1) and b(K) = w(|K|) v(K) (|K| <= p - 1),
//   phi_j = sum_{K containing j} (a + b)(K) - sum_K b(K),
// so a lane keeps sum (a + b) per high feature of the subsets it saw, one sum for its own T and one of b; a unit's
// partials are reduced once per launch by fixed butterflies and added to its own row of the partial table, which a
// last kernel sums in fixed order.  No floating-point atomics: the result is bitwise the same from call to call.
//
// Pairwise Shapley interaction index (lsspa_subsets_interactions, the INTER instantiation of the enumeration kernel):
//   I_ij = sum_{S without i, j} w2(|S|) (v(S + i + j) - v(S + i) - v(S + j) + v(S)),   w2(s) = s! (p - 2 - s)! / (p - 1)!,
// is another linear functional of the same v(K).  With alpha(k) = w2(k - 2), beta(k) = w2(k - 1), gamma(k) = w2(k) (0
// outside 0 .. p - 2) and k = |K|,
//   I_ij = T0 - T1_i - T1_j + T2_ij,   T0 = sum_K gamma v,   T1_i = sum_{K with i} (beta + gamma) v,
//   T2_ij = sum_{K with i and j} (alpha + 2 beta + gamma) v.
// T0 and T1 are kept like b and phi's sums above.  T2: a lane keeps the (alpha + 2 beta + gamma) sum of its own T and
// one per high feature -- reduced over the lanes with bit t, or bits s and t, at the end of a launch they are the
// high-low and low-low pairs; a pair of HIGH features depends on hi alone, which the whole wave shares, so the wave's
// sum of the weighted values of one high subset goes to the pairs inside hi, which are dealt over the lanes (at most
// SHH = 6 a lane) with their masks built once.  A unit's row of the partial table is then
//   [0 .. p] as above | T0 | T1 [p] | T2 [p (p - 1) / 2] (pairs i < j, row-major),
// its first p + 1 columns computed by the very operations of the phi-only kernel.
//
// Replicates (the bootstrap, k_boot.hip): launch_subsets_enum(.., reps) runs `reps` problems laid out one behind the other
// as the second grid dimension of the kernel (the REPS instantiations, rep_offset below), phi-only or with the interaction
// sums; a replicate's arithmetic is that of the one-problem kernel, operation for operation.
//
// Best subset of every size (lsspa_subsets_best, subsets_best_kernel below): the same enumeration keeps, instead of sums,
// the largest v(K) and its mask per size |K| -- a kernel of its own beside the enumeration kernel, which it leaves alone.
// Its REPS instantiation runs the replicates of a bootstrap of the selection (lsspa_boot_best_run) as the second grid
// dimension, like the enumeration kernel's.
//
// K-fold cross-validation (lsspa_cv_best, subsets_cv_best_kernel below): that kernel's sibling, which evaluates every
// high subset on the K fold problems of k_cv.hip in one step and keeps the best SUM of their values per size;
// lsspa_cv_top, subsets_cv_top_kernel: the same fold-step with subsets_top_kernel's lists, the T best sums per size.
#include "kernels.h"

namespace lsspa {
namespace {

constexpr int SQ = 6;                          // low features: one lane per low subset, 2^6 lanes = one wave
constexpr int SP = SUBSETS_MAX_P;              // 32
constexpr int SNH = SP - SQ;                   // largest number of high features
constexpr int LDM = SP + 1;                    // row stride of the compacted sweep matrix (n <= p + 1 <= 33)
constexpr int SENT = (LDM * LDM + 63) / 64;    // sweep entries a lane owns at most (18)
constexpr int ZC = SQ + 2;                     // row stride of Z: columns 0 .. q of X^T H X, then X^T h
constexpr int SHH = (SNH * (SNH - 1) / 2 + 63) / 64;   // pairs of high features a lane owns at most (6)

struct SubShared {
  double H[SP * LDM];      // test Gram, stride LDM
  double h[SP];
  double gdiag[SP];        // diagonal of G: the pivot scale
  double wa[SP + 1], wb[SP + 1];
  double M[LDM * LDM];     // compacted augmented matrix being swept
  double X[SP * (SQ + 1)]; // [e0 E] over Hs + low, stride SQ + 1
  double Y[SP * (SQ + 1)]; // H X
  double Z[(SQ + 1) * ZC]; // X^T H X | X^T h
  int idx[SP];             // compacted position -> feature
};

// Replicates (the bootstrap, k_boot.hip): replicate r = blockIdx.y of a launch has its problem r strides behind the
// launch's -- G, H: p ld, g, h: p, one 1 / ||y||^2 and one info word each, part: the table of the replicates before it.
// Those are the REPS instantiations (phi-only and INTER, whose row of the table is subsets_inter_cols(p) wide); without
// REPS the replicate is 0 at compile time and the code is what it was before replicates existed (the kernel sits at the
// edge of its register budget: see DESIGN.md).
template <bool REPS>
__device__ inline int64_t rep_offset(int64_t stride) { return REPS ? (int64_t)blockIdx.y * stride : 0; }

__device__ inline double wave_sum(double x) {
  // fixed butterfly, then lane 0's value for everyone: the same order on every call
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return __shfl(x, 0, 64);
}

// v(Hs + T) of this lane's low subset T = lane (0 for lanes >= 2^q).  Enters and leaves with the workgroup (one wave)
// in step: every shared array it writes is free when it is called and is read by nobody after it returns.
template <bool REPS>
__device__ double subset_values(SubShared& sh, const SubsetArgs& a, uint64_t hi, int lane, bool& bad) {
  const int p = a.p, q = a.q;
  const int nhs = __popcll(hi);
  if (lane < p) {
    if (lane < q)
      sh.idx[nhs + lane] = lane;
    else if ((hi >> (lane - q)) & 1ull)
      sh.idx[__popcll(hi & ((1ull << (lane - q)) - 1ull))] = lane;
  }
  const int nk = nhs + q;     // features of Hs + low
  const int n = nk + 1;       // ... and the right-hand side
  const int nn = n * n;
  const double* Gr = a.G + rep_offset<REPS>(p * a.ldg);
  const double* gr = a.g + rep_offset<REPS>(p);
  __syncthreads();
  int ea[SENT], eb[SENT];
#pragma unroll
  for (int r = 0; r < SENT; ++r) {
    const int e = lane + 64 * r;
    ea[r] = e / n;
    eb[r] = e - ea[r] * n;
    if (e < nn) {
      const int i = ea[r], j = eb[r];
      double val = 0.0;
      if (i < nk && j < nk)
        val = Gr[(int64_t)sh.idx[i] * a.ldg + sh.idx[j]];
      else if (i < nk)
        val = gr[sh.idx[i]];
      else if (j < nk)
        val = gr[sh.idx[j]];
      sh.M[i * LDM + j] = val;
    }
  }
  __syncthreads();
  // sweep the high pivots: new M_kj = M_kj / d, M_ik = -M_ik / d, M_kk = 1 / d, M_ij -= M_ik M_kj / d
  for (int k = 0; k < nhs; ++k) {
    const double d = sh.M[k * LDM + k];
    if (!(d > a.piv_tol * sh.gdiag[sh.idx[k]])) bad = true;
    const double inv = 1.0 / d;
    double nv[SENT];
#pragma unroll
    for (int r = 0; r < SENT; ++r) {
      nv[r] = 0.0;
      if (lane + 64 * r < nn) {
        const int i = ea[r], j = eb[r];
        const double mik = sh.M[i * LDM + k], mkj = sh.M[k * LDM + j];
        if (i == k)
          nv[r] = (j == k) ? inv : mkj * inv;
        else if (j == k)
          nv[r] = -mik * inv;
        else
          nv[r] = sh.M[i * LDM + j] - mik * (mkj * inv);
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SENT; ++r)
      if (lane + 64 * r < nn) sh.M[ea[r] * LDM + eb[r]] = nv[r];
    __syncthreads();
  }
  // X = [e0 E] over the nk compacted features (columns 0 .. q)
  const int nc = q + 1;
  for (int e = lane; e < nk * nc; e += 64) {
    const int i = e / nc, c = e - i * nc;
    double x;
    if (i < nhs)
      x = (c == 0) ? sh.M[i * LDM + nk] : -sh.M[i * LDM + nhs + c - 1];
    else
      x = (c - 1 == i - nhs) ? 1.0 : 0.0;
    sh.X[i * (SQ + 1) + c] = x;
  }
  __syncthreads();
  for (int e = lane; e < nk * nc; e += 64) {
    const int i = e / nc, c = e - i * nc;
    const double* Hr = sh.H + sh.idx[i] * LDM;
    double s = 0.0;
    for (int b = 0; b < nk; ++b) s += Hr[sh.idx[b]] * sh.X[b * (SQ + 1) + c];
    sh.Y[i * (SQ + 1) + c] = s;
  }
  __syncthreads();
  if (lane < nc * (nc + 1)) {
    const int c = lane / (nc + 1), c2 = lane - c * (nc + 1);
    double s = 0.0;
    if (c2 < nc)
      for (int i = 0; i < nk; ++i) s += sh.X[i * (SQ + 1) + c] * sh.Y[i * (SQ + 1) + c2];
    else
      for (int i = 0; i < nk; ++i) s += sh.X[i * (SQ + 1) + c] * sh.h[sh.idx[i]];
    sh.Z[c * ZC + (c2 < nc ? c2 : SQ + 1)] = s;
  }
  __syncthreads();
  // lane T: theta_T = S_TT^-1 g~_T with everything outside T masked to the identity
  double v = 0.0;
  if (lane < (1 << q)) {
    bool in[SQ];
#pragma unroll
    for (int t = 0; t < SQ; ++t) in[t] = (t < q) && ((lane >> t) & 1);
    double L[SQ][SQ], y[SQ];
#pragma unroll
    for (int t = 0; t < SQ; ++t) {
      const double mt = sh.M[(nhs + t) * LDM + nk];
      y[t] = in[t] ? mt : 0.0;
#pragma unroll
      for (int s = 0; s <= t; ++s) {
        const double ms = sh.M[(nhs + t) * LDM + nhs + s];
        L[t][s] = (in[t] && in[s]) ? ms : (s == t ? 1.0 : 0.0);
      }
    }
#pragma unroll
    for (int j = 0; j < SQ; ++j) {
      double d = L[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
      if (in[j] && !(d > a.piv_tol * sh.gdiag[j])) bad = true;
      const double r = 1.0 / sqrt(d);
      L[j][j] = d * r;
#pragma unroll
      for (int i = j + 1; i < SQ; ++i) {
        double s = L[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
        L[i][j] = s * r;
      }
    }
#pragma unroll
    for (int i = 0; i < SQ; ++i) {
      double s = y[i];
#pragma unroll
      for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
      y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = SQ - 1; i >= 0; --i) {
      double s = y[i];
#pragma unroll
      for (int k = i + 1; k < SQ; ++k) s -= L[k][i] * y[k];
      y[i] = s / L[i][i];                 // theta_T (exactly 0 outside T)
    }
    double f = 2.0 * sh.Z[SQ + 1] - sh.Z[0];
#pragma unroll
    for (int t = 0; t < SQ; ++t) {
      if (t < q) {
        double u = 2.0 * (sh.Z[(1 + t) * ZC + SQ + 1] - sh.Z[(1 + t) * ZC]);
#pragma unroll
        for (int s = 0; s < SQ; ++s)
          if (s < q) u -= sh.Z[(1 + t) * ZC + 1 + s] * y[s];
        f += y[t] * u;
      }
    }
    v = f * a.inv_yy[rep_offset<REPS>(1)];
  }
  return v;
}

template <bool REPS>
__device__ void load_shared(SubShared& sh, const SubsetArgs& a, int lane) {
  const int p = a.p;
  const double* Hr = a.H + rep_offset<REPS>(p * a.ldh);
  for (int e = lane; e < p * p; e += 64) {
    const int i = e / p, j = e - i * p;
    sh.H[i * LDM + j] = Hr[(int64_t)i * a.ldh + j];
  }
  if (lane < p) {
    sh.h[lane] = a.h[rep_offset<REPS>(p) + lane];
    sh.gdiag[lane] = a.G[rep_offset<REPS>(p * a.ldg) + (int64_t)lane * a.ldg + lane];
  }
  if (lane <= p) {
    sh.wa[lane] = a.w[lane];
    sh.wb[lane] = a.w[SP + 1 + lane];
  }
  for (int e = lane; e < (SQ + 1) * ZC; e += 64) sh.Z[e] = 0.0;   // rows / columns beyond q stay 0
}

// column of pair (i, j), i < j, among the p (p - 1) / 2 pairs of a row of the interactions table
__device__ inline int pair_col(int p, int i, int j) { return i * (2 * p - i - 1) / 2 + (j - i - 1); }

// INTER: the interaction sums T0, T1, T2 beside phi's (lsspa_subsets_interactions); a row of part is then
// subsets_inter_cols(p) wide.  Everything of the phi-only instantiation is in both, unchanged.
template <bool INTER, bool REPS = false>
__global__ __launch_bounds__(64) void subsets_enum_kernel(SubsetArgs a, uint64_t s0, uint64_t s1) {
  __shared__ SubShared sh;
  __shared__ double w2[INTER ? 3 * (SP + 1) : 1];   // gamma, beta + gamma, alpha + 2 beta + gamma by |K|
  const int lane = threadIdx.x;
  const int p = a.p, q = a.q, nh = p - q;
  load_shared<REPS>(sh, a, lane);
  double acc[SNH];
#pragma unroll
  for (int j = 0; j < SNH; ++j) acc[j] = 0.0;
  double c_own = 0.0, b_own = 0.0;
  // INTER only (dead code otherwise)
  double acc1[INTER ? SNH : 1], acc2[INTER ? SNH : 1], hh[SHH];
  uint32_t hm[SHH];
  double g_own = 0.0, e_own = 0.0, d_own = 0.0;
  if constexpr (INTER) {
    for (int e = lane; e < 3 * (SP + 1); e += 64) w2[e] = a.w[2 * (SP + 1) + e];
#pragma unroll
    for (int j = 0; j < SNH; ++j) acc1[j] = acc2[j] = 0.0;
    // pair number e = lane + 64 r of the nh (nh - 1) / 2 pairs j1 < j2 of high features, as a mask over hi; a slot
    // without a pair gets a mask that no hi contains (nh <= 26)
#pragma unroll
    for (int r = 0; r < SHH; ++r) {
      hh[r] = 0.0;
      int rem = lane + 64 * r, j1 = 0;
      while (j1 < nh - 1 && rem >= nh - 1 - j1) {
        rem -= nh - 1 - j1;
        ++j1;
      }
      hm[r] = (j1 < nh - 1) ? ((1u << j1) | (1u << (j1 + 1 + rem))) : 0x80000000u;
    }
  }
  bool bad = false;
  const bool live = lane < (1 << q);
  const int kt = __popc(lane);
  for (uint64_t s = s0; s < s1; ++s) {
    const uint64_t hi = (uint64_t)blockIdx.x * a.per + s;
    const double v = subset_values<REPS>(sh, a, hi, lane, bad);
    if (live) {
      const int k = __popcll(hi) + kt;
      const double c = (sh.wa[k] + sh.wb[k]) * v;
      c_own += c;
      b_own += sh.wb[k] * v;
#pragma unroll
      for (int j = 0; j < SNH; ++j)
        if (j < nh && ((hi >> j) & 1ull)) acc[j] += c;
    }
    if constexpr (INTER) {
      double d = 0.0;
      if (live) {
        const int k = __popcll(hi) + kt;
        const double e = w2[SP + 1 + k] * v;
        d = w2[2 * (SP + 1) + k] * v;
        g_own += w2[k] * v;
        e_own += e;
        d_own += d;
#pragma unroll
        for (int j = 0; j < SNH; ++j)
          if (j < nh && ((hi >> j) & 1ull)) {
            acc1[j] += e;
            acc2[j] += d;
          }
      }
      if (nh >= 2) {                          // the same for the whole wave
        const double dw = wave_sum(d);
        const uint32_t h32 = (uint32_t)hi;
#pragma unroll
        for (int r = 0; r < SHH; ++r)
          if ((h32 & hm[r]) == hm[r]) hh[r] += dw;
      }
    }
    __syncthreads();
  }
  double* part = a.part + (rep_offset<REPS>(gridDim.x) + blockIdx.x) * (INTER ? (p + 2 + p + p * (p - 1) / 2) : (p + 1));
#pragma unroll
  for (int t = 0; t < SQ; ++t) {
    if (t < q) {
      const double tot = wave_sum((live && ((lane >> t) & 1)) ? c_own : 0.0);
      if (lane == 0) part[t] += tot;
    }
  }
#pragma unroll
  for (int j = 0; j < SNH; ++j) {
    if (j < nh) {
      const double tot = wave_sum(acc[j]);
      if (lane == 0) part[q + j] += tot;
    }
  }
  const double tb = wave_sum(b_own);
  if (lane == 0) part[p] += tb;
  if constexpr (INTER) {
    double* t1 = part + p + 2;
    double* t2 = t1 + p;
    const double t0 = wave_sum(g_own);
    if (lane == 0) part[p + 1] += t0;
#pragma unroll
    for (int t = 0; t < SQ; ++t) {
      if (t < q) {
        const bool has_t = live && ((lane >> t) & 1);
        const double tot = wave_sum(has_t ? e_own : 0.0);
        if (lane == 0) t1[t] += tot;
#pragma unroll
        for (int u = 0; u < SQ; ++u) {          // low-low pairs (u, t), u < t
          if (u < t) {
            const double both = wave_sum((has_t && ((lane >> u) & 1)) ? d_own : 0.0);
            if (lane == 0) t2[pair_col(p, u, t)] += both;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < SNH; ++j) {
      if (j < nh) {
        const double tot = wave_sum(acc1[j]);
        if (lane == 0) t1[q + j] += tot;
        for (int t = 0; t < q; ++t) {           // high-low pairs (t, q + j)
          const double hl = wave_sum((live && ((lane >> t) & 1)) ? acc2[j] : 0.0);
          if (lane == 0) t2[pair_col(p, t, q + j)] += hl;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < SHH; ++r) {             // high-high pairs: every lane holds the sums of its own
      if (hm[r] != 0x80000000u) {
        const int j1 = __ffs((int)hm[r]) - 1, j2 = 31 - __clz((int)hm[r]);
        t2[pair_col(p, q + j1, q + j2)] += hh[r];
      }
    }
  }
  if (__any(bad) && lane == 0) atomicOr(a.info + rep_offset<REPS>(1), 1);
}

__global__ __launch_bounds__(64) void subsets_reduce_kernel(const double* __restrict__ part, int64_t units, int p1,
                                                            double* __restrict__ out) {
  const int j = blockIdx.x, lane = threadIdx.x;
  part += rep_offset<true>(units * p1);      // replicate blockIdx.y: its table, its sums
  out += rep_offset<true>(p1);
  double s = 0.0;
  for (int64_t u = lane; u < units; u += 64) s += part[u * p1 + j];
  s = wave_sum(s);
  if (lane == 0) out[j] = s;
}

__global__ __launch_bounds__(64) void subsets_debug_kernel(SubsetArgs a, const uint64_t* __restrict__ masks,
                                                           int64_t n, double* __restrict__ vals) {
  __shared__ SubShared sh;
  const int lane = threadIdx.x;
  load_shared<false>(sh, a, lane);
  bool bad = false;
  const uint64_t low = (1ull << a.q) - 1ull;
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint64_t m = masks[i];
    const double v = subset_values<false>(sh, a, m >> a.q, lane, bad);
    if ((uint64_t)lane == (m & low)) vals[i] = v;
    __syncthreads();
  }
  if (__any(bad) && lane == 0) atomicOr(a.info, 1);
}

// ---- best subset of every size (lsspa_subsets_best) ----
// The same units, steps and launches as subsets_enum_kernel, the same subset_values; what is kept of v(K) is not a sum
// but, per size k = |K|, the largest value and its mask (hi << q) | T.  Order: the larger value wins, on equal values
// the numerically smaller mask; a subset whose own pivot failed, or that lacks a column of `include`, is no candidate
// and NaN never wins (v > best from -inf).  The order is total, so the result does not depend on how the work is cut.
//
// Running bests: |K| = popc(hi) + popc(T) and hi = blockIdx.x per + s with per a power of two, so popc(hi) =
// popc(blockIdx.x) + popc(s): inside a unit the size class of a lane's subset is popc(s), at most log2(per) + 1 <=
// SBS = 14 classes (per <= 2^13).  A lane keeps (value, hi) per class in statically indexed registers; popc(s) is the
// same for the whole wave, so the update is one compare-select behind a scalar branch.  Within a class a lane sees its
// masks in ascending order: the strict compare keeps the smaller one.
constexpr int SBS = 14;

// (v, mask) <- the better of it and (bv, bmask) in the total order above; "no candidate" is v = -inf here (a candidate
// won a strict compare against -inf, so its value is larger), which loses against every candidate
__device__ inline void best_merge(double& v, uint32_t& mask, double bv, uint32_t bmask) {
  const bool take = bv > v || (bv == v && bmask < mask);
  v = take ? bv : v;
  mask = take ? bmask : mask;
}

__device__ inline void wave_best(double& v, uint32_t& mask) {
  // fixed butterfly; the order is total, so every lane ends with the same winner
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const uint32_t om = (uint32_t)__shfl_xor((int)mask, o, 64);
    best_merge(v, mask, ov, om);
  }
}

// a.part [units][p + 1] (values), bm [units][p + 1][2] (mask, found): unit u's best subset of every size so far; a launch
// merges its own into them (found = 0: no candidate yet, the value and mask beside it mean nothing).  One workgroup owns a row, launches are ordered by the stream: plain loads and stores.
// REPS (the bootstrap of the selection, lsspa_boot_best_run): replicate blockIdx.y reads its own problem, 1 / ||y||^2 and
// info word (rep_offset) and merges into its own rows of the tables [reps][units][p + 1] and [reps][units][p + 1][2].
// The order is total, so a replicate's result depends neither on the cut of `per` into launches nor on the replicates
// that share its launch.  The offsets are applied once, to the kernel's own copy of the arguments, and the helpers run
// as for one problem: load_shared<true> and subset_values<true> form them again at every step, which in this kernel
// (14 classes of running bests beside the sweep) costs 36 bytes of scratch a lane.  The addresses, and so the
// arithmetic, are the same.  Without REPS the code is what it was.
template <bool REPS = false>
__global__ __launch_bounds__(64) void subsets_best_kernel(SubsetArgs a, uint64_t s0, uint64_t s1, uint32_t include,
                                                          uint32_t* __restrict__ bm) {
  __shared__ SubShared sh;
  const int lane = threadIdx.x;
  const int p = a.p, q = a.q;
  if constexpr (REPS) {
    a.G += rep_offset<REPS>(p * a.ldg);
    a.H += rep_offset<REPS>(p * a.ldh);
    a.g += rep_offset<REPS>(p);
    a.h += rep_offset<REPS>(p);
    a.inv_yy += rep_offset<REPS>(1);
    a.info += rep_offset<REPS>(1);
    a.part += rep_offset<REPS>((int64_t)gridDim.x * (p + 1));
    bm += rep_offset<REPS>((int64_t)gridDim.x * (p + 1) * 2);
  }
  load_shared<false>(sh, a, lane);
  double bv[SBS];
  uint32_t bh[SBS];
#pragma unroll
  for (int j = 0; j < SBS; ++j) {
    bv[j] = -__builtin_huge_val();
    bh[j] = 0u;
  }
  const uint32_t inc_lo = include & ((1u << q) - 1u), inc_hi = include >> q;     // q >= 1
  const bool lane_ok = lane < (1 << q) && ((uint32_t)lane & inc_lo) == inc_lo;
  bool any_bad = false;
  for (uint64_t s = s0; s < s1; ++s) {
    const uint64_t hi = (uint64_t)blockIdx.x * a.per + s;
    bool bad = false;                         // this subset's own pivots: the high ones the wave's, the low ones the lane's
    const double v = subset_values<false>(sh, a, hi, lane, bad);
    any_bad |= bad;
    const uint32_t h32 = (uint32_t)hi;
    const bool cand = lane_ok && !bad && (h32 & inc_hi) == inc_hi;
    const int cls = __popcll(s);
#pragma unroll
    for (int j = 0; j < SBS; ++j)
      if (cls == j && cand && v > bv[j]) {
        bv[j] = v;
        bh[j] = h32;
      }
    __syncthreads();
  }
  double* rv = a.part + (int64_t)blockIdx.x * (p + 1);
  uint32_t* rm = bm + (int64_t)blockIdx.x * (p + 1) * 2;
  // the sizes this unit can hold: popc(unit) + popc(s) + popc(T), s < per (a power of two), T < 2^q
  const int k0 = __popc(blockIdx.x), k1 = min(p, k0 + __popcll(a.per - 1) + q);
  const int base = k0 + __popc(lane);                       // |K| of this lane's class 0
  for (int k = k0; k <= k1; ++k) {
    double v = -__builtin_huge_val();
    uint32_t mask = 0u;
#pragma unroll
    for (int j = 0; j < SBS; ++j)
      if (base + j == k) {
        v = bv[j];
        mask = (bh[j] << q) | (uint32_t)lane;
      }
    wave_best(v, mask);
    if (lane == 0 && v > -__builtin_huge_val()) {
      if (rm[2 * k + 1] != 0u) best_merge(v, mask, rv[k], rm[2 * k]);
      rv[k] = v;
      rm[2 * k] = mask;
      rm[2 * k + 1] = 1u;
    }
  }
  if (__any(any_bad) && lane == 0) atomicOr(a.info, 1);
}

// out_v [p + 1], out_m [p + 1][2]: the best over the units, one workgroup per size, the units dealt over the lanes in a
// fixed order (any order gives the same winner).  Replicate blockIdx.y: its rows of the tables, and a result `ostride`
// doubles (out_v) or pairs (out_m) behind the first replicate's.
__global__ __launch_bounds__(64) void subsets_best_reduce_kernel(const double* __restrict__ bv,
                                                                 const uint32_t* __restrict__ bm, int64_t units, int p1,
                                                                 double* __restrict__ out_v,
                                                                 uint32_t* __restrict__ out_m, int64_t ostride) {
  const int k = blockIdx.x, lane = threadIdx.x;
  bv += rep_offset<true>(units * p1);
  bm += rep_offset<true>(units * p1 * 2);
  out_v += rep_offset<true>(ostride);
  out_m += rep_offset<true>(ostride * 2);
  double v = -__builtin_huge_val();
  uint32_t mask = 0u;
  for (int64_t u = lane; u < units; u += 64) {
    const int64_t e = u * p1 + k;
    if (bm[2 * e + 1] != 0u) best_merge(v, mask, bv[e], bm[2 * e]);
  }
  wave_best(v, mask);
  if (lane == 0) {
    out_v[k] = v;
    out_m[2 * k] = mask;
    out_m[2 * k + 1] = v > -__builtin_huge_val() ? 1u : 0u;
  }
}

// ---- the T best subsets of every size (lsspa_subsets_top) ----
// subsets_best_kernel's sibling: the same units, steps and launches, the same load_shared and subset_values, the same
// candidates (the subset contains `include`, its own pivots passed, its value is above -inf, so never NaN); what is kept
// per size k = |K| is not one winner but the T best, 1 <= T <= SUBSETS_TOP_MAX, in the same total order -- the larger
// value first, on equal values the numerically smaller mask.  Masks are unique, so the order is strict and the T best of
// any collection of subsets are one definite list: the result depends neither on the cut into units and launches nor
// on the order of the inserts.
//
// Lists: |K| = popc(unit) + popc(s) + popc(T), so a unit meets at most STS = SBS + SQ = 20 sizes, popc(unit) + j with
// j = popc(s) + popc(lane).  Per such j it keeps a sorted list of up to T (value, mask) and a count -- in LDS, not in
// registers: a lane's size changes from step to step and a list belongs to the wave, not to a lane.  The lists are
// dynamic LDS, 12 T + 4 bytes a size beside SubShared (T = 1: 320 B, seven workgroups a CU as before; T = 16: 3920 B,
// six).  A launch loads them from the unit's rows of the table and stores them back at its end (one workgroup owns a
// row, launches are ordered by the stream: plain loads and stores); the counts are cleared before the first launch, the
// entries need not be.
// Every step, fast path: a lane reads its list's count and last entry, compares, and one ballot says whether any lane
// has something to insert.  Once the lists have filled almost no step does.  Slow path, the same for the whole wave:
// the lowest lane of the ballot broadcasts (value, mask, j); lane t < T holds entry t of that list, rank = how many
// entries come before the new one, entries from `rank` on move down by one shuffle and the one that falls off position
// T - 1 is dropped; then the lanes still waiting compare again with the list as it now is.
constexpr int STS = SBS + SQ;

// does (v, m) come before (ov, om) in the total order?
__device__ inline bool top_before(double v, uint32_t m, double ov, uint32_t om) { return v > ov || (v == ov && m < om); }

// bytes of dynamic LDS: values [STS][T], masks [STS][T], counts [STS]
constexpr size_t top_lds_bytes(int T) { return (size_t)STS * T * 12 + (size_t)STS * 4; }

// a.part [units][p + 1][T] (values), tm [units][p + 1][T] (masks), tc [units][p + 1] (counts): unit u's T best of every
// size so far, best first
__global__ __launch_bounds__(64) void subsets_top_kernel(SubsetArgs a, uint64_t s0, uint64_t s1, uint32_t include, int T,
                                                         uint32_t* __restrict__ tm, int32_t* __restrict__ tc) {
  __shared__ SubShared sh;
  extern __shared__ double top_lds[];
  double* lv = top_lds;
  uint32_t* lm = reinterpret_cast<uint32_t*>(lv + STS * T);
  int* lc = reinterpret_cast<int*>(lm + STS * T);
  const int lane = threadIdx.x;
  const int p = a.p, q = a.q;
  load_shared<false>(sh, a, lane);
  // the sizes this unit can hold: k0 + j, j < ns (popc(s) + popc(T) with s < per, T < 2^q, and no more than p)
  const int k0 = __popc(blockIdx.x);
  const int ns = min(p - k0, __popcll(a.per - 1) + q) + 1;
  double* gv = a.part + ((int64_t)blockIdx.x * (p + 1) + k0) * T;
  uint32_t* gm = tm + ((int64_t)blockIdx.x * (p + 1) + k0) * T;
  int32_t* gc = tc + (int64_t)blockIdx.x * (p + 1) + k0;
  for (int e = lane; e < ns * T; e += 64) {
    const int j = e / T;
    if (e - j * T < gc[j]) {
      lv[e] = gv[e];
      lm[e] = gm[e];
    }
  }
  if (lane < ns) lc[lane] = gc[lane];
  // (subset_values passes a barrier before anything below reads the lists)
  const uint32_t inc_lo = include & ((1u << q) - 1u), inc_hi = include >> q;     // q >= 1
  const bool lane_ok = lane < (1 << q) && ((uint32_t)lane & inc_lo) == inc_lo;
  const int jl = lane_ok ? __popc(lane) : 0;
  bool any_bad = false;
  for (uint64_t s = s0; s < s1; ++s) {
    const uint64_t hi = (uint64_t)blockIdx.x * a.per + s;
    bool bad = false;                         // this subset's own pivots, as in subsets_best_kernel
    const double v = subset_values<false>(sh, a, hi, lane, bad);
    any_bad |= bad;
    const uint32_t h32 = (uint32_t)hi;
    const uint32_t m = (h32 << q) | (uint32_t)lane;
    const int j = __popcll(s) + jl;           // < ns for every lane that can be a candidate
    // a candidate that belongs into its size's list as it is now: the list is not full, or its last entry comes later
    auto wanted = [&]() {
      const int c = lc[j];
      return c < T || top_before(v, m, lv[j * T + T - 1], lm[j * T + T - 1]);
    };
    bool want = lane_ok && !bad && (h32 & inc_hi) == inc_hi && v > -__builtin_huge_val() && wanted();
    for (uint64_t todo = __ballot(want); todo != 0ull; todo = __ballot(want)) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      const double nv = __shfl(v, src, 64);
      const uint32_t nm = (uint32_t)__shfl((int)m, src, 64);
      const int nj = __shfl(j, src, 64);
      double* rv = lv + nj * T;
      uint32_t* rm = lm + nj * T;
      const int c = lc[nj];
      const bool have = lane < c;             // c <= T <= 16: lane t holds entry t
      const double ev = have ? rv[lane] : 0.0;
      const uint32_t em = have ? rm[lane] : 0u;
      const int rank = __popcll(__ballot(have && top_before(ev, em, nv, nm)));
      const double pv = __shfl_up(ev, 1, 64);
      const uint32_t pm = (uint32_t)__shfl_up((int)em, 1, 64);
      const int nc = min(c + 1, T);
      if (lane >= rank && lane < nc) {        // a lane writes the entry it read: no other lane's
        rv[lane] = lane == rank ? nv : pv;
        rm[lane] = lane == rank ? nm : pm;
      }
      if (lane == 0) lc[nj] = nc;
      __syncthreads();
      if (lane == src) want = false;
      want = want && wanted();
    }
    __syncthreads();
  }
  for (int e = lane; e < ns * T; e += 64) {
    const int j = e / T;
    if (e - j * T < lc[j]) {
      gv[e] = lv[e];
      gm[e] = lm[e];
    }
  }
  if (lane < ns) gc[lane] = lc[lane];
  if (__any(any_bad) && lane == 0) atomicOr(a.info, 1);
}

// out_v [p + 1][T], out_m [p + 1][T], out_c [p + 1]: per size the T best over all units' lists in the same order, NaN / 0
// past the count.  One workgroup of TRT threads per size; a thread owns the units u = thread + TRT i.  A unit's list is
// sorted, so the best entry it still has is its first one not yet taken: LDS keeps per unit how many were taken and how
// many there are.  T rounds: every thread takes the best of its units' heads, fixed butterflies give the best of all
// (the order is strict, so every thread sees the same winner whatever the order of the merges), which is written as
// the next rank; the one thread that held it moves that unit on.  "No head" is -inf, which loses against every entry.
constexpr int TRT = 256, TRU = 32;            // units <= TRT TRU = 8192
__global__ __launch_bounds__(TRT) void subsets_top_reduce_kernel(const double* __restrict__ tv,
                                                                 const uint32_t* __restrict__ tm,
                                                                 const int32_t* __restrict__ tc, int units, int p1, int T,
                                                                 double* __restrict__ out_v,
                                                                 uint32_t* __restrict__ out_m,
                                                                 int32_t* __restrict__ out_c) {
  __shared__ double wv[TRT / 64];
  __shared__ uint32_t wm[TRT / 64];
  __shared__ uint8_t pos[TRT * TRU], cnt[TRT * TRU];      // of unit u: entries taken, entries there are (<= 16)
  const int k = blockIdx.x, tid = threadIdx.x;
  for (int u = tid; u < units; u += TRT) {                // a unit's two bytes are its thread's alone
    pos[u] = 0;
    cnt[u] = (uint8_t)tc[(int64_t)u * p1 + k];
  }
  int n = 0;
  for (; n < T; ++n) {
    double v = -__builtin_huge_val();
    uint32_t mask = 0u;
    int bu = -1;
    for (int u = tid; u < units; u += TRT) {
      const int t = pos[u];
      if (t < cnt[u]) {
        const int64_t e = ((int64_t)u * p1 + k) * T + t;
        const double ev = tv[e];
        const uint32_t em = tm[e];
        if (bu < 0 || top_before(ev, em, v, mask)) {
          v = ev;
          mask = em;
          bu = u;
        }
      }
    }
    const uint32_t own = mask;                            // (with bu >= 0) this thread's candidate
    wave_best(v, mask);
    if ((tid & 63) == 0) {
      wv[tid >> 6] = v;
      wm[tid >> 6] = mask;
    }
    __syncthreads();
    v = wv[0];
    mask = wm[0];
#pragma unroll
    for (int w = 1; w < TRT / 64; ++w) best_merge(v, mask, wv[w], wm[w]);
    __syncthreads();
    if (!(v > -__builtin_huge_val())) break;              // no head left: the same for every thread
    if (tid == 0) {
      out_v[k * T + n] = v;
      out_m[k * T + n] = mask;
    }
    if (bu >= 0 && own == mask) ++pos[bu];                // masks of one size are unique: one thread
  }
  if (tid == 0) {
    out_c[k] = n;
    for (int r = n; r < T; ++r) {
      out_v[k * T + r] = __builtin_nan("");
      out_m[k * T + r] = 0u;
    }
  }
}

// ---- best subset of every size by the K-fold cross-validated value (lsspa_cv_best) ----
// subsets_best_kernel's sibling: the same units, steps and launches, running bests per class popc(s), best_merge /
// wave_best, table layout and subsets_best_reduce_kernel.  What is compared is not one problem's v(K) but
//   v_cv(K) = v_0(K) + v_1(K) + ... + v_{F-1}(K)   (fp64, in this order),
// v_f the value subset_values gives for fold problem f: the F reduced problems lie one behind the other at the dense
// replicate stride (SubsetArgs), and one step evaluates its high subset on all of them before the compare.  A subset is
// a candidate only if it contains `include` and its own pivots passed in EVERY fold; a failed pivot raises the info word
// of the fold it failed in.
// The test side reaches the wave per fold-step: H_f, h_f and the diagonal of G_f are staged from memory (they stay in
// the L2: F (p^2 + 2 p) doubles) into the one SubShared the workgroup has, then subset_values<false> runs on fold f's
// arguments -- the same code on other addresses, so v_f has the bits the one-problem kernels give for problem f.  The
// workgroup's LDS is SubShared's, as its siblings': seven one-wave workgroups a CU whatever F is ("K-fold
// cross-validation", has the alternatives and why they lose).  The staging costs p^2 / 64 <= 16 loads a lane a
// fold-step beside the up to 18 of the sweep matrix that subset_values does anyway.
__device__ inline SubsetArgs fold_args(const SubsetArgs& a, int f) {
  SubsetArgs b = a;
  b.G += (int64_t)f * a.p * a.ldg;
  b.H += (int64_t)f * a.p * a.ldh;
  b.g += (int64_t)f * a.p;
  b.h += (int64_t)f * a.p;
  b.inv_yy += f;
  return b;
}

// H, h and the pivot scale of one fold into sh; the caller's last barrier is behind every read of them
__device__ inline void load_fold(SubShared& sh, const SubsetArgs& a, int lane) {
  const int p = a.p;
  for (int e = lane; e < p * p; e += 64) {
    const int i = e / p, j = e - i * p;
    sh.H[i * LDM + j] = a.H[(int64_t)i * a.ldh + j];
  }
  if (lane < p) {
    sh.h[lane] = a.h[lane];
    sh.gdiag[lane] = a.G[(int64_t)lane * a.ldg + lane];
  }
}

// a.part [units][p + 1], bm [units][p + 1][2] as subsets_best_kernel's; a.info [F]
__global__ __launch_bounds__(64, 2) void subsets_cv_best_kernel(SubsetArgs a, int F, uint64_t s0, uint64_t s1,
                                                             uint32_t include, uint32_t* __restrict__ bm) {
  __shared__ SubShared sh;
  const int lane = threadIdx.x;
  const int p = a.p, q = a.q;
  for (int e = lane; e < (SQ + 1) * ZC; e += 64) sh.Z[e] = 0.0;   // rows / columns beyond q stay 0
  double bv[SBS];
  uint32_t bh[SBS];
#pragma unroll
  for (int j = 0; j < SBS; ++j) {
    bv[j] = -__builtin_huge_val();
    bh[j] = 0u;
  }
  const uint32_t inc_lo = include & ((1u << q) - 1u), inc_hi = include >> q;     // q >= 1
  const bool lane_ok = lane < (1 << q) && ((uint32_t)lane & inc_lo) == inc_lo;
  uint32_t bad_folds = 0u;                    // bit f: a pivot of fold f failed in a subset this lane saw
  for (uint64_t s = s0; s < s1; ++s) {
    const uint64_t hi = (uint64_t)blockIdx.x * a.per + s;
    double v = 0.0;
    bool bad_any = false;                     // this subset's own pivots, over the folds
#pragma unroll 1
    for (int f = 0; f < F; ++f) {
      const SubsetArgs af = fold_args(a, f);
      load_fold(sh, af, lane);
      bool bad = false;
      const double vf = subset_values<false>(sh, af, hi, lane, bad);
      v = f == 0 ? vf : v + vf;
      bad_any |= bad;
      bad_folds |= bad ? (1u << f) : 0u;
      __syncthreads();
    }
    const uint32_t h32 = (uint32_t)hi;
    const bool cand = lane_ok && !bad_any && (h32 & inc_hi) == inc_hi;
    const int cls = __popcll(s);
#pragma unroll
    for (int j = 0; j < SBS; ++j)
      if (cls == j && cand && v > bv[j]) {
        bv[j] = v;
        bh[j] = h32;
      }
  }
  double* rv = a.part + (int64_t)blockIdx.x * (p + 1);
  uint32_t* rm = bm + (int64_t)blockIdx.x * (p + 1) * 2;
  const int k0 = __popc(blockIdx.x), k1 = min(p, k0 + __popcll(a.per - 1) + q);
  const int base = k0 + __popc(lane);                       // |K| of this lane's class 0
  for (int k = k0; k <= k1; ++k) {
    double v = -__builtin_huge_val();
    uint32_t mask = 0u;
#pragma unroll
    for (int j = 0; j < SBS; ++j)
      if (base + j == k) {
        v = bv[j];
        mask = (bh[j] << q) | (uint32_t)lane;
      }
    wave_best(v, mask);
    if (lane == 0 && v > -__builtin_huge_val()) {
      if (rm[2 * k + 1] != 0u) best_merge(v, mask, rv[k], rm[2 * k]);
      rv[k] = v;
      rm[2 * k] = mask;
      rm[2 * k + 1] = 1u;
    }
  }
  for (int f = 0; f < F; ++f)
    if (__any((bad_folds >> f) & 1u) && lane == 0) atomicOr(a.info + f, 1);
}

// test hook and the winners' per-fold values: vals[i] = v_cv(masks[i]), vfold[i][f] = v_f(masks[i]) (vfold may be
// null), by the very fold-step of subsets_cv_best_kernel
__global__ __launch_bounds__(64, 2) void subsets_cv_debug_kernel(SubsetArgs a, int F, const uint64_t* __restrict__ masks,
                                                              int64_t n, double* __restrict__ vals,
                                                              double* __restrict__ vfold) {
  __shared__ SubShared sh;
  const int lane = threadIdx.x;
  for (int e = lane; e < (SQ + 1) * ZC; e += 64) sh.Z[e] = 0.0;
  uint32_t bad_folds = 0u;
  const uint64_t low = (1ull << a.q) - 1ull;
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint64_t m = masks[i];
    const bool mine = (uint64_t)lane == (m & low);
    double v = 0.0;
#pragma unroll 1
    for (int f = 0; f < F; ++f) {
      const SubsetArgs af = fold_args(a, f);
      load_fold(sh, af, lane);
      bool bad = false;
      const double vf = subset_values<false>(sh, af, m >> a.q, lane, bad);
      v = f == 0 ? vf : v + vf;
      bad_folds |= (bad && mine) ? (1u << f) : 0u;
      if (mine && vfold) vfold[i * F + f] = vf;
      __syncthreads();
    }
    if (mine) vals[i] = v;
  }
  for (int f = 0; f < F; ++f)
    if (__any((bad_folds >> f) & 1u) && lane == 0) atomicOr(a.info + f, 1);
}

// ---- the T best subsets of every size by the K-fold cross-validated value (lsspa_cv_top) ----
// The product of the two kernels above it: subsets_cv_best_kernel's fold-step (the same units, steps and launches, fold_args /
// load_fold / subset_values<false> per fold, v = v_0 + v_1 + ... in fold order, so every v_f and every sum has the bits
// subsets_cv_debug_kernel gives for that mask; the same candidates -- valid lane, `include`, own pivots passed in EVERY
// fold -- and the same info words) and subsets_top_kernel's lists (STS sizes a unit, T entries and a count each, in
// dynamic LDS beside the one SubShared; loaded from the unit's rows of the table at the start of a launch and stored
// back at its end; wanted(), the ballot and the rank-and-shift insert as there; top_before's strict order, so the
// lists depend on no cut of the work).  The table is subsets_top_kernel's and subsets_top_reduce_kernel merges it.
// A candidate's sum must also be above -inf, so it is never NaN.
// The lists stay in LDS over the fold loop, which restages H, h and the pivot scale into SubShared F times a step and
// touches nothing else of the workgroup's LDS; one list check a step stands against F sweeps.  Barriers: every
// fold-step ends in one, so the lists' first reader (wanted(), after the folds) is behind the loads above the loop,
// and every insert ends in one as in subsets_top_kernel; the step needs no barrier of its own behind the inserts,
// because what follows (load_fold) writes SubShared only and the next reader of the lists is F barriers away.
__global__ __launch_bounds__(64, 2) void subsets_cv_top_kernel(SubsetArgs a, int F, uint64_t s0, uint64_t s1,
                                                            uint32_t include, int T, uint32_t* __restrict__ tm,
                                                            int32_t* __restrict__ tc) {
  __shared__ SubShared sh;
  extern __shared__ double top_lds[];
  double* lv = top_lds;
  uint32_t* lm = reinterpret_cast<uint32_t*>(lv + STS * T);
  int* lc = reinterpret_cast<int*>(lm + STS * T);
  const int lane = threadIdx.x;
  const int p = a.p, q = a.q;
  for (int e = lane; e < (SQ + 1) * ZC; e += 64) sh.Z[e] = 0.0;   // rows / columns beyond q stay 0
  // the sizes this unit can hold: k0 + j, j < ns (popc(s) + popc(T) with s < per, T < 2^q, and no more than p)
  const int k0 = __popc(blockIdx.x);
  const int ns = min(p - k0, __popcll(a.per - 1) + q) + 1;
  double* gv = a.part + ((int64_t)blockIdx.x * (p + 1) + k0) * T;
  uint32_t* gm = tm + ((int64_t)blockIdx.x * (p + 1) + k0) * T;
  int32_t* gc = tc + (int64_t)blockIdx.x * (p + 1) + k0;
  for (int e = lane; e < ns * T; e += 64) {
    const int j = e / T;
    if (e - j * T < gc[j]) {
      lv[e] = gv[e];
      lm[e] = gm[e];
    }
  }
  if (lane < ns) lc[lane] = gc[lane];
  const uint32_t inc_lo = include & ((1u << q) - 1u), inc_hi = include >> q;     // q >= 1
  const bool lane_ok = lane < (1 << q) && ((uint32_t)lane & inc_lo) == inc_lo;
  const int jl = lane_ok ? __popc(lane) : 0;
  uint32_t bad_folds = 0u;                    // bit f: a pivot of fold f failed in a subset this lane saw
  for (uint64_t s = s0; s < s1; ++s) {
    const uint64_t hi = (uint64_t)blockIdx.x * a.per + s;
    double v = 0.0;
    bool bad_any = false;                     // this subset's own pivots, over the folds
#pragma unroll 1
    for (int f = 0; f < F; ++f) {
      const SubsetArgs af = fold_args(a, f);
      load_fold(sh, af, lane);
      bool bad = false;
      const double vf = subset_values<false>(sh, af, hi, lane, bad);
      v = f == 0 ? vf : v + vf;
      bad_any |= bad;
      bad_folds |= bad ? (1u << f) : 0u;
      __syncthreads();
    }
    const uint32_t h32 = (uint32_t)hi;
    const uint32_t m = (h32 << q) | (uint32_t)lane;
    const int j = __popcll(s) + jl;           // < ns for every lane that can be a candidate
    // a candidate that belongs into its size's list as it is now: the list is not full, or its last entry comes later
    auto wanted = [&]() {
      const int c = lc[j];
      return c < T || top_before(v, m, lv[j * T + T - 1], lm[j * T + T - 1]);
    };
    bool want = lane_ok && !bad_any && (h32 & inc_hi) == inc_hi && v > -__builtin_huge_val() && wanted();
    for (uint64_t todo = __ballot(want); todo != 0ull; todo = __ballot(want)) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      const double nv = __shfl(v, src, 64);
      const uint32_t nm = (uint32_t)__shfl((int)m, src, 64);
      const int nj = __shfl(j, src, 64);
      double* rv = lv + nj * T;
      uint32_t* rm = lm + nj * T;
      const int c = lc[nj];
      const bool have = lane < c;             // c <= T <= 16: lane t holds entry t
      const double ev = have ? rv[lane] : 0.0;
      const uint32_t em = have ? rm[lane] : 0u;
      const int rank = __popcll(__ballot(have && top_before(ev, em, nv, nm)));
      const double pv = __shfl_up(ev, 1, 64);
      const uint32_t pm = (uint32_t)__shfl_up((int)em, 1, 64);
      const int nc = min(c + 1, T);
      if (lane >= rank && lane < nc) {        // a lane writes the entry it read: no other lane's
        rv[lane] = lane == rank ? nv : pv;
        rm[lane] = lane == rank ? nm : pm;
      }
      if (lane == 0) lc[nj] = nc;
      __syncthreads();
      if (lane == src) want = false;
      want = want && wanted();
    }
  }
  // (every write of the lists is behind a barrier: the loads' the fold-steps', an insert's its own)
  for (int e = lane; e < ns * T; e += 64) {
    const int j = e / T;
    if (e - j * T < lc[j]) {
      gv[e] = lv[e];
      gm[e] = lm[e];
    }
  }
  if (lane < ns) gc[lane] = lc[lane];
  for (int f = 0; f < F; ++f)
    if (__any((bad_folds >> f) & 1u) && lane == 0) atomicOr(a.info + f, 1);
}

// H = Ft Ft^T [p][p] (stride p) and h = Ft ytil (appended) of the rect-mode test factor: one workgroup per entry, its
// 256 threads strided over the m columns, then a fixed tree (the same sums on every call; m may be up to 2^20 through
// lsspa_set_reduced).  Entries (i, j) and (j, i) both form the product of rows min(i, j) and max(i, j) in the same
// order, so H is exactly symmetric.
__global__ __launch_bounds__(256) void subsets_test_gram_kernel(const double* __restrict__ Ft, int64_t ldf,
                                                                const double* __restrict__ ytil, int p, int m,
                                                                double* __restrict__ Hh) {
  __shared__ double red[256];
  const int e = blockIdx.x;                  // grid = p (p + 1): entry (i, j), j == p is h
  const int i = e / (p + 1), j = e - i * (p + 1);
  const int a = (j < p && j < i) ? j : i, b = (j < p && j < i) ? i : j;   // (a, b) with a <= b or b == p
  const double* ra = Ft + (int64_t)a * ldf;
  const double* rb = (b < p) ? Ft + (int64_t)b * ldf : ytil;
  double s = 0.0;
  for (int r = threadIdx.x; r < m; r += 256) s += ra[r] * rb[r];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (j < p)
      Hh[i * p + j] = red[0];
    else
      Hh[p * p + i] = red[0];
  }
}

bool args_ok(const SubsetArgs& a) {
  return a.p >= 1 && a.p <= SP && a.q == (a.p < SQ ? a.p : SQ) && a.G && a.g && a.H && a.h && a.w && a.info &&
         a.inv_yy && a.ldg >= a.p && a.ldh >= a.p;
}

}  // namespace

int subsets_low_features(int p) { return p < SQ ? p : SQ; }

int subsets_inter_cols(int p) { return p + 2 + p + p * (p - 1) / 2; }

hipError_t launch_subsets_enum(const SubsetArgs& a, uint64_t units, uint64_t s0, uint64_t s1, bool inter,
                               hipStream_t st, int reps) {
  if (!args_ok(a) || !a.part || units < 1 || s1 <= s0 || s1 > a.per) return hipErrorInvalidValue;
  // replicates: the caller vouches for `reps` problems, tables, info words behind the first
  if (reps < 1 || reps > 65535) return hipErrorInvalidValue;
  // every high subset index of the launch must exist: unit u covers [u per, (u + 1) per) of 2^(p - q)
  const int nh = a.p - a.q;
  if (units * a.per != (1ull << nh) || units > (1ull << 31)) return hipErrorInvalidValue;
  if (inter && reps > 1)
    hipLaunchKernelGGL((subsets_enum_kernel<true, true>), dim3((unsigned)units, (unsigned)reps), dim3(64), 0, st, a, s0,
                       s1);
  else if (inter)
    hipLaunchKernelGGL(subsets_enum_kernel<true>, dim3((unsigned)units), dim3(64), 0, st, a, s0, s1);
  else if (reps > 1)
    hipLaunchKernelGGL((subsets_enum_kernel<false, true>), dim3((unsigned)units, (unsigned)reps), dim3(64), 0, st, a, s0,
                       s1);
  else
    hipLaunchKernelGGL(subsets_enum_kernel<false>, dim3((unsigned)units), dim3(64), 0, st, a, s0, s1);
  return hipGetLastError();
}

hipError_t launch_subsets_reduce(const double* part, int64_t units, int cols, double* out, hipStream_t st, int reps) {
  if (!part || !out || units < 1 || cols < 2 || cols > subsets_inter_cols(SP) || reps < 1 || reps > 65535)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(subsets_reduce_kernel, dim3(cols, (unsigned)reps), dim3(64), 0, st, part, units, cols, out);
  return hipGetLastError();
}

hipError_t launch_subsets_best(const SubsetArgs& a, uint64_t units, uint64_t s0, uint64_t s1, uint32_t include,
                               uint32_t* bm, hipStream_t st, int reps) {
  if (!args_ok(a) || !a.part || !bm || units < 1 || s1 <= s0 || s1 > a.per) return hipErrorInvalidValue;
  // replicates: the caller vouches for `reps` problems, rows of both tables and info words behind the first
  if (reps < 1 || reps > 65535) return hipErrorInvalidValue;
  const int nh = a.p - a.q;
  if (units * a.per != (1ull << nh) || units > (1ull << 31)) return hipErrorInvalidValue;
  // the size classes of a unit are popc(s), s < per: per a power of two (it is: units per = 2^nh) of at most SBS - 1 bits
  if (a.per > (1ull << (SBS - 1))) return hipErrorInvalidValue;
  if (a.p < 32 && (include >> a.p) != 0u) return hipErrorInvalidValue;
  if (reps > 1)
    hipLaunchKernelGGL(subsets_best_kernel<true>, dim3((unsigned)units, (unsigned)reps), dim3(64), 0, st, a, s0, s1,
                       include, bm);
  else
    hipLaunchKernelGGL(subsets_best_kernel<false>, dim3((unsigned)units), dim3(64), 0, st, a, s0, s1, include, bm);
  return hipGetLastError();
}

hipError_t launch_subsets_best_reduce(const double* bv, const uint32_t* bm, int64_t units, int p, double* out_v,
                                      uint32_t* out_m, hipStream_t st, int reps, int64_t out_stride) {
  if (!bv || !bm || !out_v || !out_m || units < 1 || p < 1 || p > SP || reps < 1 || reps > 65535 ||
      (reps > 1 && out_stride < p + 1))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(subsets_best_reduce_kernel, dim3(p + 1, (unsigned)reps), dim3(64), 0, st, bv, bm, units, p + 1,
                     out_v, out_m, out_stride);
  return hipGetLastError();
}

hipError_t launch_subsets_top(const SubsetArgs& a, uint64_t units, uint64_t s0, uint64_t s1, uint32_t include, int T,
                              uint32_t* tm, int32_t* tc, hipStream_t st) {
  if (!args_ok(a) || !a.part || !tm || !tc || units < 1 || s1 <= s0 || s1 > a.per) return hipErrorInvalidValue;
  if (T < 1 || T > SUBSETS_TOP_MAX) return hipErrorInvalidValue;
  const int nh = a.p - a.q;
  if (units * a.per != (1ull << nh) || units > (1ull << 31)) return hipErrorInvalidValue;
  // the sizes of a unit are popc(s) + popc(lane), s < per: per a power of two of at most SBS - 1 bits, STS lists
  if (a.per > (1ull << (SBS - 1))) return hipErrorInvalidValue;
  if (a.p < 32 && (include >> a.p) != 0u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(subsets_top_kernel, dim3((unsigned)units), dim3(64), top_lds_bytes(T), st, a, s0, s1, include, T,
                     tm, tc);
  return hipGetLastError();
}

hipError_t launch_subsets_top_reduce(const double* tv, const uint32_t* tm, const int32_t* tc, int64_t units, int p, int T,
                                     double* out_v, uint32_t* out_m, int32_t* out_c, hipStream_t st) {
  if (!tv || !tm || !tc || !out_v || !out_m || !out_c || units < 1 || units > TRT * TRU || p < 1 || p > SP || T < 1 ||
      T > SUBSETS_TOP_MAX)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(subsets_top_reduce_kernel, dim3(p + 1), dim3(TRT), 0, st, tv, tm, tc, (int)units, p + 1, T, out_v,
                     out_m, out_c);
  return hipGetLastError();
}

size_t subsets_cv_lds_bytes() { return sizeof(SubShared); }

hipError_t launch_subsets_cv_best(const SubsetArgs& a, int folds, uint64_t units, uint64_t s0, uint64_t s1,
                                  uint32_t include, uint32_t* bm, hipStream_t st) {
  if (!args_ok(a) || !a.part || !bm || units < 1 || s1 <= s0 || s1 > a.per) return hipErrorInvalidValue;
  // the caller vouches for `folds` problems and info words behind the first, as launch_subsets_best's for its replicates
  if (folds < 2 || folds > CV_MAX_FOLDS) return hipErrorInvalidValue;
  const int nh = a.p - a.q;
  if (units * a.per != (1ull << nh) || units > (1ull << 31)) return hipErrorInvalidValue;
  if (a.per > (1ull << (SBS - 1))) return hipErrorInvalidValue;
  if (a.p < 32 && (include >> a.p) != 0u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(subsets_cv_best_kernel, dim3((unsigned)units), dim3(64), 0, st, a, folds, s0, s1, include, bm);
  return hipGetLastError();
}

size_t subsets_cv_top_lds_bytes(int T) { return sizeof(SubShared) + top_lds_bytes(T); }

hipError_t launch_subsets_cv_top(const SubsetArgs& a, int folds, uint64_t units, uint64_t s0, uint64_t s1,
                                 uint32_t include, int T, uint32_t* tm, int32_t* tc, hipStream_t st) {
  if (!args_ok(a) || !a.part || !tm || !tc || units < 1 || s1 <= s0 || s1 > a.per) return hipErrorInvalidValue;
  if (T < 1 || T > SUBSETS_TOP_MAX) return hipErrorInvalidValue;
  // the caller vouches for `folds` problems and info words behind the first, as launch_subsets_cv_best's does
  if (folds < 2 || folds > CV_MAX_FOLDS) return hipErrorInvalidValue;
  const int nh = a.p - a.q;
  if (units * a.per != (1ull << nh) || units > (1ull << 31)) return hipErrorInvalidValue;
  // the sizes of a unit are popc(s) + popc(lane), s < per: per a power of two of at most SBS - 1 bits, STS lists
  if (a.per > (1ull << (SBS - 1))) return hipErrorInvalidValue;
  if (a.p < 32 && (include >> a.p) != 0u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(subsets_cv_top_kernel, dim3((unsigned)units), dim3(64), top_lds_bytes(T), st, a, folds, s0, s1,
                     include, T, tm, tc);
  return hipGetLastError();
}

hipError_t launch_subsets_cv_debug(const SubsetArgs& a, int folds, const uint64_t* masks, int64_t n, double* vals,
                                   double* vfold, hipStream_t st) {
  if (!args_ok(a) || !masks || !vals || n < 1 || folds < 2 || folds > CV_MAX_FOLDS) return hipErrorInvalidValue;
  const int64_t grid = n < 4096 ? n : 4096;
  hipLaunchKernelGGL(subsets_cv_debug_kernel, dim3((unsigned)grid), dim3(64), 0, st, a, folds, masks, n, vals, vfold);
  return hipGetLastError();
}

hipError_t launch_subsets_debug(const SubsetArgs& a, const uint64_t* masks, int64_t n, double* vals, hipStream_t st) {
  if (!args_ok(a) || !masks || !vals || n < 1) return hipErrorInvalidValue;
  const int64_t grid = n < 4096 ? n : 4096;
  hipLaunchKernelGGL(subsets_debug_kernel, dim3((unsigned)grid), dim3(64), 0, st, a, masks, n, vals);
  return hipGetLastError();
}

hipError_t launch_subsets_test_gram(const double* Ft, int64_t ldf, const double* ytil, int p, int m, double* Hh,
                                    hipStream_t st) {
  if (!Ft || !ytil || !Hh || p < 1 || p > GROUPS_MAX_P || m < 1 || ldf < m) return hipErrorInvalidValue;
  hipLaunchKernelGGL(subsets_test_gram_kernel, dim3(p * (p + 1)), dim3(256), 0, st, Ft, ldf, ytil, p, m, Hh);
  return hipGetLastError();
}

}  // namespace lsspa
