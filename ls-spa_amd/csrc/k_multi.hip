// Exact attribution of many responses at once (lsspa_multi_shapley, p <= 32): the enumeration of k_subsets.hip with
// MULTI_RB right-hand sides carried through one sweep.  fp64 throughout.
//
// For a high subset Hs the sweep of the pivots of Hs, E = [-A^-1 B; I], H E and W = E^T H E, and every lane's masked
// 6 x 6 Cholesky factor depend on G and H alone (k_subsets.hip's header has the algebra).  A response r owns one
// column of the swept matrix (A^-1 g_Hs in the Hs rows, g~ in the low rows), one column e0_r of X and H e0_r of Y, the
// scalars f0_r = 2 e0_r.h_r - e0_r^T H e0_r and r_r[t] = 2 (E_t.h_r - E_t^T H e0_r), two 6-long triangular solves and
//   v_r(Hs + T) = (f0_r + theta^T (r_r - W theta)) / ||y_r||^2,   theta = S_TT^-1 g~_r,T.
// A wave carries a CHUNK of MULTI_RB responses per pass; the chunks are the second grid dimension.  The swept matrix is
// nk rows by nk + MULTI_RB columns (the row g^T of the one-response kernel's augmented matrix is never read there, and
// is not kept here).  Slots of the last chunk beyond the responses given compute on zero columns and store nothing.
//
// Accumulators: per response a lane keeps the (a + b) sum and the b sum of its own low subset T (k_subsets.hip's c_own,
// b_own), and lane j the (a + b) sum of HIGH feature j: the sum over a high subset's lanes of (wa + wb) v is butterflied
// once per response and subset, and the lanes whose feature is in hi add it.  3 MULTI_RB accumulators a lane, where
// MULTI_RB copies of the one-response kernel's 28 would not fit.  All sums run in a fixed order; no floating-point atomics.
//
// Independence: a response's arithmetic reads G, H and its own columns, and is the same operation sequence in every
// slot and chunk -- its bits do not depend on where it stands, on the other responses or on how a run is cut.
#include "kernels.h"

namespace lsspa {
namespace {

constexpr int SQ = 6;                          // low features: one lane per low subset, 2^6 lanes = one wave
constexpr int SP = MULTI_MAX_P;                // 32
constexpr int RB = MULTI_RB;                   // responses a wave carries per pass
constexpr int LDM = SP + RB + 1;               // row stride of the sweep matrix (nk + RB <= 40 columns; odd)
constexpr int SENT = (SP * (SP + RB) + 63) / 64;   // sweep entries a lane owns at most (20)
constexpr int LDX = RB + SQ + 1;               // row stride of X, Y: columns 0 .. RB-1 e0_r, RB .. RB+q-1 E (odd)
constexpr int LDH = SP + 1;                    // row stride of H
constexpr int ZR = SQ + 2;                     // row stride of the per-response scalars: r_r[0 .. 5], f0_r

struct MultiShared {
  double H[SP * LDH];      // test Gram
  double gdiag[SP];        // diagonal of G: the pivot scale
  double wa[SP + 1], wb[SP + 1];
  double g[SP * RB];       // [feature][slot] of the chunk's responses (0 beyond them)
  double h[SP * RB];
  double iyy[RB];          // 1 / ||y_r||^2 (0 beyond the chunk's responses)
  double M[SP * LDM];      // compacted [G_KK | g_K,r] being swept
  double X[SP * LDX];      // [e0_r | E] over Hs + low
  double Y[SP * LDX];      // H X
  double W[SQ * SQ];       // E^T H E
  double Zr[RB * ZR];      // r_r, f0_r
  int idx[SP];             // compacted position -> feature
};

__device__ inline double wave_sum(double x) {
  // fixed butterfly, then lane 0's value for everyone: the same order on every call
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return __shfl(x, 0, 64);
}

// responses of chunk blockIdx.y that exist: 1 .. RB
__device__ inline int chunk_responses(const MultiArgs& a) {
  const int left = a.count - (int)blockIdx.y * RB;
  return left < RB ? left : RB;
}

__device__ void load_shared(MultiShared& sh, const MultiArgs& a, int lane) {
  const int p = a.p;
  for (int e = lane; e < p * p; e += 64) {
    const int i = e / p, j = e - i * p;
    sh.H[i * LDH + j] = a.H[(int64_t)i * a.ldh + j];
  }
  if (lane < p) sh.gdiag[lane] = a.G[(int64_t)lane * a.ldg + lane];
  if (lane <= p) {
    sh.wa[lane] = a.w[lane];
    sh.wb[lane] = a.w[SP + 1 + lane];
  }
  const int nv = chunk_responses(a);
  const int64_t r0 = (int64_t)blockIdx.y * RB;
  for (int e = lane; e < p * RB; e += 64) {
    const int i = e / RB, r = e - i * RB;
    sh.g[e] = r < nv ? a.g[(r0 + r) * p + i] : 0.0;
    sh.h[e] = r < nv ? a.h[(r0 + r) * p + i] : 0.0;
  }
  if (lane < RB) sh.iyy[lane] = lane < nv ? a.inv_yy[r0 + lane] : 0.0;
  for (int e = lane; e < SQ * SQ; e += 64) sh.W[e] = 0.0;     // rows / columns beyond q stay 0
  for (int e = lane; e < RB * ZR; e += 64) sh.Zr[e] = 0.0;
}

// v[r] = v_r(Hs + T) of this lane's low subset T = lane for the chunk's RB slots (0 for lanes >= 2^q).  Enters and
// leaves with the workgroup (one wave) in step: every shared array it writes is free when it is called and is read by
// nobody after it returns.
__device__ void multi_values(MultiShared& sh, const MultiArgs& a, uint64_t hi, int lane, bool& bad, double (&v)[RB]) {
  const int p = a.p, q = a.q;
  const int nhs = __popcll(hi);
  if (lane < p) {
    if (lane < q)
      sh.idx[nhs + lane] = lane;
    else if ((hi >> (lane - q)) & 1ull)
      sh.idx[__popcll(hi & ((1ull << (lane - q)) - 1ull))] = lane;
  }
  const int nk = nhs + q;     // features of Hs + low: rows of the sweep matrix
  const int n = nk + RB;      // ... its columns
  const int nn = nk * n;
  __syncthreads();
  int ea[SENT], eb[SENT];
#pragma unroll
  for (int r = 0; r < SENT; ++r) {
    const int e = lane + 64 * r;
    ea[r] = e / n;
    eb[r] = e - ea[r] * n;
    if (e < nn) {
      const int i = ea[r], j = eb[r];
      sh.M[i * LDM + j] = (j < nk) ? a.G[(int64_t)sh.idx[i] * a.ldg + sh.idx[j]] : sh.g[sh.idx[i] * RB + (j - nk)];
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
  // X = [e0_r | E] over the nk compacted features
  const int nc = RB + q;
  for (int e = lane; e < nk * nc; e += 64) {
    const int i = e / nc, c = e - i * nc;
    double x;
    if (i < nhs)
      x = (c < RB) ? sh.M[i * LDM + nk + c] : -sh.M[i * LDM + nhs + c - RB];
    else
      x = (c - RB == i - nhs) ? 1.0 : 0.0;
    sh.X[i * LDX + c] = x;
  }
  __syncthreads();
  for (int e = lane; e < nk * nc; e += 64) {
    const int i = e / nc, c = e - i * nc;
    const double* Hr = sh.H + sh.idx[i] * LDH;
    double s = 0.0;
    for (int b = 0; b < nk; ++b) s += Hr[sh.idx[b]] * sh.X[b * LDX + c];
    sh.Y[i * LDX + c] = s;
  }
  __syncthreads();
  // W = E^T H E (shared), then per response r_r[t] = 2 (E_t.h_r - E_t^T H e0_r) and f0_r = 2 e0_r.h_r - e0_r^T H e0_r
  if (lane < q * q) {
    const int t = lane / q, s2 = lane - t * q;
    double s = 0.0;
    for (int i = 0; i < nk; ++i) s += sh.X[i * LDX + RB + t] * sh.Y[i * LDX + RB + s2];
    sh.W[t * SQ + s2] = s;
  }
  if (lane < RB * (q + 1)) {
    const int r = lane / (q + 1), c = lane - r * (q + 1);
    const int col = (c < q) ? RB + c : r;                  // E_c, or e0_r for the last task
    double zh = 0.0, zy = 0.0;
    for (int i = 0; i < nk; ++i) {
      const double x = sh.X[i * LDX + col];
      zh += x * sh.h[sh.idx[i] * RB + r];
      zy += x * sh.Y[i * LDX + r];
    }
    sh.Zr[r * ZR + (c < q ? c : SQ)] = (c < q) ? 2.0 * (zh - zy) : 2.0 * zh - zy;
  }
  __syncthreads();
  // lane T: the masked 6 x 6 factor once, then theta_T = S_TT^-1 g~_T and the quadratic form per response
#pragma unroll
  for (int r = 0; r < RB; ++r) v[r] = 0.0;
  if (lane < (1 << q)) {
    bool in[SQ];
#pragma unroll
    for (int t = 0; t < SQ; ++t) in[t] = (t < q) && ((lane >> t) & 1);
    double L[SQ][SQ], ri[SQ];
#pragma unroll
    for (int t = 0; t < SQ; ++t) {
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
      const double rs = 1.0 / sqrt(d);
      ri[j] = rs;                          // 1 / L_jj: the solves multiply
#pragma unroll
      for (int i = j + 1; i < SQ; ++i) {
        double s = L[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
        L[i][j] = s * rs;
      }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      double y[SQ];
#pragma unroll
      for (int t = 0; t < SQ; ++t) {
        const double mt = sh.M[(nhs + t) * LDM + nk + r];
        y[t] = in[t] ? mt : 0.0;
      }
#pragma unroll
      for (int i = 0; i < SQ; ++i) {
        double s = y[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
        y[i] = s * ri[i];
      }
#pragma unroll
      for (int i = SQ - 1; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < SQ; ++k) s -= L[k][i] * y[k];
        y[i] = s * ri[i];                  // theta_T (exactly 0 outside T)
      }
      double f = sh.Zr[r * ZR + SQ];
#pragma unroll
      for (int t = 0; t < SQ; ++t) {
        if (t < q) {
          double u = sh.Zr[r * ZR + t];
#pragma unroll
          for (int s = 0; s < SQ; ++s)
            if (s < q) u -= sh.W[t * SQ + s] * y[s];
          f += y[t] * u;
        }
      }
      v[r] = f * sh.iyy[r];
    }
  }
}

// part [chunks][RB][units][p + 1]: the row of (chunk, slot, unit); gridDim.x = units
__device__ inline double* part_row(const MultiArgs& a, int r) {
  return a.part + ((((int64_t)blockIdx.y * RB + r) * gridDim.x) + blockIdx.x) * (a.p + 1);
}

__global__ __launch_bounds__(64) void multi_enum_kernel(MultiArgs a, uint64_t s0, uint64_t s1) {
  __shared__ MultiShared sh;
  const int lane = threadIdx.x;
  const int p = a.p, q = a.q, nh = p - q;
  load_shared(sh, a, lane);
  double c_own[RB], b_own[RB], h_own[RB];     // own low subset: (a + b), b; high feature `lane`: (a + b)
#pragma unroll
  for (int r = 0; r < RB; ++r) c_own[r] = b_own[r] = h_own[r] = 0.0;
  bool bad = false;
  const bool live = lane < (1 << q);
  const int kt = __popc(lane);
  for (uint64_t s = s0; s < s1; ++s) {
    const uint64_t hi = (uint64_t)blockIdx.x * a.per + s;
    double v[RB];
    multi_values(sh, a, hi, lane, bad, v);
    const int k = __popcll(hi) + kt;
    const double wc = live ? sh.wa[k] + sh.wb[k] : 0.0, wbk = live ? sh.wb[k] : 0.0;
    const bool mine = lane < nh && ((hi >> lane) & 1ull);
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      // The contraction is spelled out: left to the compiler, c_own += wc v became an fma in the one slot (7) where c
      // was not kept in a register and a multiply and an add in the others, and a response's bits depended on its slot.
#pragma clang fp contract(off)
      const double c = wc * v[r];
      c_own[r] += c;
      b_own[r] = __builtin_fma(wbk, v[r], b_own[r]);
      if (nh > 0) {                            // the same for the whole wave
        const double tot = wave_sum(c);
        if (mine) h_own[r] += tot;
      }
    }
    __syncthreads();
  }
  const int nv = chunk_responses(a);
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    if (r < nv) {                              // the same for the whole wave
      double* part = part_row(a, r);
#pragma unroll
      for (int t = 0; t < SQ; ++t) {
        if (t < q) {
          const double tot = wave_sum((live && ((lane >> t) & 1)) ? c_own[r] : 0.0);
          if (lane == 0) part[t] += tot;
        }
      }
      if (lane < nh) part[q + lane] += h_own[r];
      const double tb = wave_sum(b_own[r]);
      if (lane == 0) part[p] += tb;
    }
  }
  if (__any(bad) && lane == 0) atomicOr(a.info, 1);
}

// vals [n][m]: the chunk's slots that exist go to columns r0 + chunk RB + slot
__global__ __launch_bounds__(64) void multi_debug_kernel(MultiArgs a, const uint64_t* __restrict__ masks, int64_t n,
                                                         double* __restrict__ vals, int m, int r0) {
  __shared__ MultiShared sh;
  const int lane = threadIdx.x;
  load_shared(sh, a, lane);
  bool bad = false;
  const uint64_t low = (1ull << a.q) - 1ull;
  const int nv = chunk_responses(a);
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint64_t mk = masks[i];
    double v[RB];
    multi_values(sh, a, mk >> a.q, lane, bad, v);
    if ((uint64_t)lane == (mk & low)) {
#pragma unroll
      for (int r = 0; r < RB; ++r)
        if (r < nv) vals[i * m + r0 + (int)blockIdx.y * RB + r] = v[r];
    }
    __syncthreads();
  }
  if (__any(bad) && lane == 0) atomicOr(a.info, 1);
}

bool args_ok(const MultiArgs& a) {
  return a.p >= 1 && a.p <= SP && a.q == (a.p < SQ ? a.p : SQ) && a.G && a.g && a.H && a.h && a.w && a.info &&
         a.inv_yy && a.ldg >= a.p && a.ldh >= a.p && a.count >= 1;
}

}  // namespace

hipError_t launch_multi_enum(const MultiArgs& a, uint64_t units, uint64_t s0, uint64_t s1, hipStream_t st) {
  if (!args_ok(a) || !a.part || units < 1 || s1 <= s0 || s1 > a.per) return hipErrorInvalidValue;
  const int nh = a.p - a.q;
  if (units * a.per != (1ull << nh) || units > (1ull << 31)) return hipErrorInvalidValue;
  const int chunks = (a.count + RB - 1) / RB;
  if (chunks > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(multi_enum_kernel, dim3((unsigned)units, (unsigned)chunks), dim3(64), 0, st, a, s0, s1);
  return hipGetLastError();
}

hipError_t launch_multi_debug(const MultiArgs& a, const uint64_t* masks, int64_t n, double* vals, int m, int r0,
                              hipStream_t st) {
  if (!args_ok(a) || !masks || !vals || n < 1 || r0 < 0 || r0 + a.count > m) return hipErrorInvalidValue;
  const int chunks = (a.count + RB - 1) / RB;
  if (chunks > 65535) return hipErrorInvalidValue;
  const int64_t grid = n < 4096 ? n : 4096;
  hipLaunchKernelGGL(multi_debug_kernel, dim3((unsigned)grid, (unsigned)chunks), dim3(64), 0, st, a, masks, n, vals, m,
                     r0);
  return hipGetLastError();
}

}  // namespace lsspa
