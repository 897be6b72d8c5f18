// Exact attribution of many responses at once over GROUPS of columns (lsspa_multi_groups_shapley, g <= 32 groups,
// p <= 64 columns, an always-included baseline): the enumeration of k_groups.hip with MULTI_RB right-hand sides carried
// through one elimination.  fp64 throughout.  The product of that file and k_multi.hip; their headers have the algebra.
//
// For a high subset Hs the Gauss-Jordan elimination of the pivots of B + cols(Hs), E = [-A^-1 C; I], H E, W = E^T H E and
// every lane's masked 6 x 6 Cholesky factor depend on G, H and the labels alone.  A response r owns one column of the
// eliminated matrix (A^-1 g_r in the pivot rows, g~_r in the low rows), one column e0_r of X and H e0_r of Y, the scalars
// f0_r = 2 e0_r.h_r - e0_r^T H e0_r and r_r[t] = 2 (E_t.h_r - E_t^T H e0_r), two 6-long triangular solves and
//   u_r(Hs + T) = (f0_r + theta^T (r_r - W theta)) / ||y_r||^2,   theta = S_TT^-1 g~_r,T.
// One workgroup of four waves owns a high subset at a time, as in k_groups.hip; a CHUNK of MULTI_RB responses rides
// through it, and the chunks are the second grid dimension, as in k_multi.hip.  The matrix is nk <= 64 rows by
// nk + MULTI_RB columns.  Slots of the last chunk beyond the responses given compute on zero columns and store nothing.
//
// The last step -- lane T of a wave masks S to the low groups in T, factors it and solves per response -- is spread over
// MG_WAVES waves: wave w takes the chunk's responses w RW .. w RW + RW - 1 (RW = MULTI_RB / MG_WAVES) and repeats the
// 6 x 6 factor.  A response's operation sequence is the same in every slot and wave.  ("Many responses over
// groups", has the measurement behind the value of MG_WAVES.)
//
// Accumulators, as k_multi.hip's: per response a lane keeps the (a + b) sum and the b sum of its own low subset T, and
// lane j the (a + b) sum of HIGH group j: the sum over a high subset's lanes of (wa + wb) u is butterflied once per
// response and subset, and the lanes whose group is in hi add it.  All sums run in a fixed order; no floating-point
// atomics.
//
// Independence: a response's arithmetic reads G, H, the layout and its own columns, and is the same operation sequence
// in every slot, wave and chunk -- its bits do not depend on where it stands, on the other responses or on how a run is
// cut.
#include "kernels.h"

namespace lsspa {
namespace {

#ifndef LSSPA_MG_WAVES
#define LSSPA_MG_WAVES 4
#endif

constexpr int GQ = GROUPS_LOW_COLS;            // low columns at most: the register-resident Cholesky
constexpr int GP = GROUPS_MAX_P;               // 64
constexpr int GG = GROUPS_MAX_G;               // 32
constexpr int RB = MULTI_RB;                   // responses a workgroup carries per pass
constexpr int NT = 256;                        // four waves
constexpr int MG_WAVES = LSSPA_MG_WAVES;       // waves that share the last step
constexpr int RW = RB / MG_WAVES;              // ... responses each of them takes
static_assert(MG_WAVES >= 1 && MG_WAVES <= NT / 64 && RW * MG_WAVES == RB, "the waves share the chunk evenly");
constexpr int LDM = GP + RB + 1;               // row stride of the matrix (nk + RB <= 72 columns; odd)
constexpr int LDX = RB + GQ + 1;               // row stride of X, Y: columns 0 .. RB-1 e0_r, RB .. RB+ql-1 E (odd)
constexpr int XW = (RB + GQ + 3) / 4;          // columns of Y a wave forms at most (4)
constexpr int ZR = GQ + 2;                     // row stride of the per-response scalars: r_r[0 .. 5], f0_r

struct MGShared {
  double M[GP * LDM];      // compacted [G_KK | g_K,r] being eliminated
  double X[GP * LDX];      // [e0_r | E]
  double Y[GP * LDX];      // H X
  double h[GP * RB];       // [column][slot] of the chunk's responses (0 beyond them)
  double W[GQ * GQ];       // E^T H E
  double Zr[RB * ZR];      // r_r, f0_r
  double iyy[RB];          // 1 / ||y_r||^2 (0 beyond the chunk's responses)
  double gdiag[GP];        // diagonal of G: the pivot scale
  double wa[GG + 1], wb[GG + 1];
  int idx[GP];             // compacted position -> column
  int cols[GP];            // the layout (GroupLayout::tab)
  int colgrp[GP];
  int colin[GP];
  int hsize[GG];
  int lgrp[GQ + 2];
};

__device__ inline double wave_sum(double x) {
  // fixed butterfly, then lane 0's value for everyone: the same order on every call
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return __shfl(x, 0, 64);
}

// responses of chunk blockIdx.y that exist: 1 .. RB
__device__ inline int chunk_responses(const MultiGroupArgs& a) {
  const int left = a.count - (int)blockIdx.y * RB;
  return left < RB ? left : RB;
}

__device__ void load_shared(MGShared& sh, const MultiGroupArgs& a, int tid) {
  const int p = a.p;
  if (tid < p) {
    sh.gdiag[tid] = a.G[(int64_t)tid * a.ldg + tid];
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
  const int nv = chunk_responses(a);
  const int64_t r0 = (int64_t)blockIdx.y * RB;
  for (int e = tid; e < p * RB; e += NT) {
    const int i = e / RB, r = e - i * RB;
    sh.h[e] = r < nv ? a.h[(r0 + r) * p + i] : 0.0;
  }
  if (tid < RB) sh.iyy[tid] = tid < nv ? a.inv_yy[r0 + tid] : 0.0;
  for (int e = tid; e < GQ * GQ; e += NT) sh.W[e] = 0.0;     // rows / columns beyond ql stay 0
  for (int e = tid; e < RB * ZR; e += NT) sh.Zr[e] = 0.0;
  __syncthreads();
}

// v[r] = u_r(Hs + T) of this thread's low subset T = lane for the responses wv RW + r of the chunk, in the waves
// wv < MG_WAVES (0 elsewhere and for lanes >= 2^gl).  Enters and leaves with the workgroup in step: every shared array it
// writes is free when it is called and is read by nobody after it returns.
__device__ void multi_group_values(MGShared& sh, const MultiGroupArgs& a, uint64_t hi, int tid, bool& bad,
                                   double (&v)[RW]) {
  const int p = a.p, ql = a.ql, nb = a.nb, gh = a.gh;
  const int wv = tid >> 6, lane = tid & 63;
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
  const int nk = nhs + ql;    // columns of B + Hs + low: rows of M
  const int n = nk + RB;      // ... its columns: nk of G, then the chunk's right-hand sides
  __syncthreads();
  const int nv = chunk_responses(a);
  const int64_t r0 = (int64_t)blockIdx.y * RB;
  for (int i = wv; i < nk; i += 4) {
    const int ci = sh.idx[i];
    for (int j = lane; j < n; j += 64) {
      double x;
      if (j < nk)
        x = a.G[(int64_t)ci * a.ldg + sh.idx[j]];
      else
        x = (j - nk < nv) ? a.g[(r0 + (j - nk)) * p + ci] : 0.0;
      sh.M[i * LDM + j] = x;
    }
  }
  __syncthreads();
  // Gauss-Jordan on the pivots 0 .. nhs-1, columns right of the pivot only (k_groups.hip): column j belongs to wave
  // (j - k - 1) % 4 of step k, column k itself is not written in step k, and the barrier separates the steps.
  for (int k = 0; k < nhs; ++k) {
    const double d = sh.M[k * LDM + k];
    if (!(d > a.piv_tol * sh.gdiag[sh.idx[k]])) bad = true;
    const double inv = 1.0 / d;
    if (lane < nk) {
      const double mik = sh.M[lane * LDM + k];
      for (int j = k + 1 + wv; j < n; j += 4) {
        const double mkj = sh.M[k * LDM + j] * inv;
        const double mij = sh.M[lane * LDM + j];
        sh.M[lane * LDM + j] = (lane == k) ? mkj : mij - mik * mkj;
      }
    }
    __syncthreads();
  }
  // X = [e0_r | E] over the nk compacted columns
  const int nc = RB + ql;
  for (int e = tid; e < nk * nc; e += NT) {
    const int i = e / nc, c = e - i * nc;
    double x;
    if (i < nhs)
      x = (c < RB) ? sh.M[i * LDM + nk + c] : -sh.M[i * LDM + nhs + c - RB];
    else
      x = (c - RB == i - nhs) ? 1.0 : 0.0;
    sh.X[i * LDX + c] = x;
  }
  __syncthreads();
  // Y = H X: lane = row i, wave wv takes columns wv, wv + 4, ...; H_ib is read as H_bi, a contiguous run of row b
  if (lane < nk) {
    const double* Hc = a.H + sh.idx[lane];
    double s[XW];
#pragma unroll
    for (int u = 0; u < XW; ++u) s[u] = 0.0;
    for (int b = 0; b < nk; ++b) {
      const double hv = Hc[(int64_t)sh.idx[b] * a.ldh];
#pragma unroll
      for (int u = 0; u < XW; ++u)
        if (wv + 4 * u < nc) s[u] += hv * sh.X[b * LDX + wv + 4 * u];
    }
#pragma unroll
    for (int u = 0; u < XW; ++u)
      if (wv + 4 * u < nc) sh.Y[lane * LDX + wv + 4 * u] = s[u];
  }
  __syncthreads();
  // W = E^T H E (the first wave), and per response r_r[t] = 2 (E_t.h_r - E_t^T H e0_r), f0_r = 2 e0_r.h_r - e0_r^T H e0_r
  // (the second: RB (ql + 1) <= 56 tasks)
  if (tid < ql * ql) {
    const int t = tid / ql, s2 = tid - t * ql;
    double s = 0.0;
    for (int i = 0; i < nk; ++i) s += sh.X[i * LDX + RB + t] * sh.Y[i * LDX + RB + s2];
    sh.W[t * GQ + s2] = s;
  }
  if (wv == 1 && lane < RB * (ql + 1)) {
    const int r = lane / (ql + 1), c = lane - r * (ql + 1);
    const int col = (c < ql) ? RB + c : r;                 // E_c, or e0_r for the last task
    double zh = 0.0, zy = 0.0;
    for (int i = 0; i < nk; ++i) {
      const double x = sh.X[i * LDX + col];
      zh += x * sh.h[sh.idx[i] * RB + r];
      zy += x * sh.Y[i * LDX + r];
    }
    sh.Zr[r * ZR + (c < ql ? c : GQ)] = (c < ql) ? 2.0 * (zh - zy) : 2.0 * zh - zy;
  }
  __syncthreads();
  // lane T of a wave: the masked 6 x 6 factor once, then theta_T = S_TT^-1 g~_T and the quadratic form per response
#pragma unroll
  for (int r = 0; r < RW; ++r) v[r] = 0.0;
  if (wv < MG_WAVES && lane < (1 << a.gl)) {
    bool in[GQ];
#pragma unroll
    for (int t = 0; t < GQ; ++t) in[t] = (t < ql) && ((lane >> sh.lgrp[t]) & 1);
    double L[GQ][GQ], ri[GQ];
#pragma unroll
    for (int t = 0; t < GQ; ++t) {
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
      const double rs = 1.0 / sqrt(d);
      ri[j] = rs;                          // 1 / L_jj: the solves multiply
#pragma unroll
      for (int i = j + 1; i < GQ; ++i) {
        double s = L[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
        L[i][j] = s * rs;
      }
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const int slot = wv * RW + r;
      double y[GQ];
#pragma unroll
      for (int t = 0; t < GQ; ++t) {
        const double mt = (t < ql) ? sh.M[(nhs + t) * LDM + nk + slot] : 0.0;
        y[t] = in[t] ? mt : 0.0;
      }
#pragma unroll
      for (int i = 0; i < GQ; ++i) {
        double s = y[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
        y[i] = s * ri[i];
      }
#pragma unroll
      for (int i = GQ - 1; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < GQ; ++k) s -= L[k][i] * y[k];
        y[i] = s * ri[i];                  // theta_T (exactly 0 outside T)
      }
      double f = sh.Zr[slot * ZR + GQ];
#pragma unroll
      for (int t = 0; t < GQ; ++t) {
        if (t < ql) {
          double u = sh.Zr[slot * ZR + t];
#pragma unroll
          for (int s = 0; s < GQ; ++s)
            if (s < ql) u -= sh.W[t * GQ + s] * y[s];
          f += y[t] * u;
        }
      }
      v[r] = f * sh.iyy[slot];
    }
  }
}

// part [chunks][RB][units][g + 1]: the row of (chunk, slot, unit); gridDim.x = units
__device__ inline double* part_row(const MultiGroupArgs& a, int slot) {
  return a.part + ((((int64_t)blockIdx.y * RB + slot) * gridDim.x) + blockIdx.x) * (a.ng + 1);
}

__global__ __launch_bounds__(NT) void multi_groups_enum_kernel(MultiGroupArgs a, uint64_t s0, uint64_t s1) {
  __shared__ MGShared sh;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int ng = a.ng, gl = a.gl, gh = a.gh;
  load_shared(sh, a, tid);
  double c_own[RW], b_own[RW], h_own[RW];     // own low subset: (a + b), b; high group `lane`: (a + b)
#pragma unroll
  for (int r = 0; r < RW; ++r) c_own[r] = b_own[r] = h_own[r] = 0.0;
  bool bad = false;
  const bool live = wv < MG_WAVES && lane < (1 << gl);
  const int kt = __popc(lane);
  for (uint64_t s = s0; s < s1; ++s) {
    const uint64_t hi = (uint64_t)blockIdx.x * a.per + s;
    double v[RW];
    multi_group_values(sh, a, hi, tid, bad, v);
    if (wv < MG_WAVES) {                       // the same for the whole wave
      const int k = __popcll(hi) + kt;
      const double wc = live ? sh.wa[k] + sh.wb[k] : 0.0, wbk = live ? sh.wb[k] : 0.0;
      const bool mine = lane < gh && ((hi >> lane) & 1ull);
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        // The contraction is spelled out, as in k_multi.hip: left to the compiler, c_own += wc v became an fma in the
        // slot where c was not kept in a register and a multiply and an add in the other.
#pragma clang fp contract(off)
        const double c = wc * v[r];
        c_own[r] += c;
        b_own[r] = __builtin_fma(wbk, v[r], b_own[r]);
        if (gh > 0) {                          // the same for the whole wave
          const double tot = wave_sum(c);
          if (mine) h_own[r] += tot;
        }
      }
    }
    __syncthreads();
  }
  const int nv = chunk_responses(a);
  if (wv < MG_WAVES) {
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const int slot = wv * RW + r;
      if (slot < nv) {                         // the same for the whole wave
        double* part = part_row(a, slot);
#pragma unroll
        for (int t = 0; t < GQ; ++t) {
          if (t < gl) {
            const double tot = wave_sum((live && ((lane >> t) & 1)) ? c_own[r] : 0.0);
            if (lane == 0) part[t] += tot;
          }
        }
        if (lane < gh) part[gl + lane] += h_own[r];
        const double tb = wave_sum(b_own[r]);
        if (lane == 0) part[ng] += tb;
      }
    }
  }
  if (__any(bad) && lane == 0) atomicOr(a.info, 1);
}

// vals [n][m]: the chunk's slots that exist go to columns r0 + chunk RB + slot; masks in the layout's own numbering
__global__ __launch_bounds__(NT) void multi_groups_debug_kernel(MultiGroupArgs a, const uint64_t* __restrict__ masks,
                                                                int64_t n, double* __restrict__ vals, int m, int r0) {
  __shared__ MGShared sh;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  load_shared(sh, a, tid);
  bool bad = false;
  const uint64_t low = (1ull << a.gl) - 1ull;
  const int nv = chunk_responses(a);
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint64_t mk = masks[i];
    double v[RW];
    multi_group_values(sh, a, mk >> a.gl, tid, bad, v);
    if (wv < MG_WAVES && (uint64_t)lane == (mk & low)) {
#pragma unroll
      for (int r = 0; r < RW; ++r)
        if (wv * RW + r < nv) vals[i * m + r0 + (int)blockIdx.y * RB + wv * RW + r] = v[r];
    }
    __syncthreads();
  }
  if (__any(bad) && lane == 0) atomicOr(a.info, 1);
}

bool args_ok(const MultiGroupArgs& a) {
  return a.p >= 1 && a.p <= GP && a.ng >= 1 && a.ng <= GG && a.gl >= 0 && a.gl <= GQ && a.gh >= 0 &&
         a.gl + a.gh == a.ng && a.ql >= a.gl && a.ql <= GQ && a.nb >= 0 && a.nb + a.ql <= a.p && a.G && a.g && a.H &&
         a.h && a.inv_yy && a.w && a.tab && a.info && a.ldg >= a.p && a.ldh >= a.p && a.count >= 1;
}

}  // namespace

hipError_t launch_multi_groups_enum(const MultiGroupArgs& a, uint64_t units, uint64_t s0, uint64_t s1, hipStream_t st) {
  if (!args_ok(a) || !a.part || units < 1 || s1 <= s0 || s1 > a.per) return hipErrorInvalidValue;
  // every high subset index of the launch must exist: unit u covers [u per, (u + 1) per) of 2^gh
  if (units * a.per != (1ull << a.gh) || units > (1ull << 31)) return hipErrorInvalidValue;
  const int chunks = (a.count + RB - 1) / RB;
  if (chunks > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(multi_groups_enum_kernel, dim3((unsigned)units, (unsigned)chunks), dim3(NT), 0, st, a, s0, s1);
  return hipGetLastError();
}

hipError_t launch_multi_groups_debug(const MultiGroupArgs& a, const uint64_t* masks, int64_t n, double* vals, int m,
                                     int r0, hipStream_t st) {
  if (!args_ok(a) || !masks || !vals || n < 1 || r0 < 0 || r0 + a.count > m) return hipErrorInvalidValue;
  const int chunks = (a.count + RB - 1) / RB;
  if (chunks > 65535) return hipErrorInvalidValue;
  const int64_t grid = n < 4096 ? n : 4096;
  hipLaunchKernelGGL(multi_groups_debug_kernel, dim3((unsigned)grid, (unsigned)chunks), dim3(NT), 0, st, a, masks, n,
                     vals, m, r0);
  return hipGetLastError();
}

}  // namespace lsspa
