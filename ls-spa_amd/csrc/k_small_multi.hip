// Sampled attribution of MANY responses on one design matrix (p <= 104, fp64): the LDS-resident kernel of k_small.hip
// with MLIFT_RB = 8 augmented rows instead of one.  Of an ordering's work
//     G_pi = L L^T,  H_pi = L_t L_t^T,  V = L^-1 L_t                                   O(p^3), the same for every response
//     z_r = L^-1 g_r[pi],  y~_r = L_t^-1 h_r[pi],  the lift scan over V                 O(p^2) per response
// only the second line belongs to a response, and in the fused kernel z and y~ are simply the augmented rows of the two
// matrices: rows p .. p + 7 of the training matrix hold g_r[pi], rows p .. p + 7 of the test matrix h_r[pi], for the eight
// responses of the workgroup's chunk.  One workgroup per (ordering, chunk of responses); the gather, both factorisations
// and the V solve run once, the lift scan once per response.
//
// The augmented rows carry right-hand sides only: a right-looking factorisation never feeds them back into rows < p, and
// their own trailing 8 x 8 corner (aug I - Z Z^T, Z the eight z rows) is never read.  Its pivots are kept positive by the
// host's choice of aug (multi_lift_launch_ok's callers: aug > the sum of the eight ||z_r||^2 -- the corner is then
// positive definite and no NaN can arise in it), and they are tested against zero, not against the relative threshold:
// only the pivots j < p of either matrix can raise LSSPA_INFO_NOT_PD.  A response whose Schur complement is exactly
// zero (y in the span of X) is therefore as good as any other.  A short last chunk pads with identity rows, as the
// rows below p + 8 are.
//
// Layout in LDS as in k_small.hip (lower 16 x 16 blocks, XOR-swizzled columns): nb = ceil((p + 8) / 16) <= 7 block rows,
// two triangles of 28 blocks = 112 KB, plus the eight saved z and y~ vectors (the V solve overwrites the test matrix's
// augmented rows, the lift terms the training matrix's).  At nb = 8 the triangles alone are 144 KB: p <= 104.
//
// What a response's bits depend on: G, H, the ordering, its own g_r, h_r, yy_r, p and its slot r mod 8 -- the other
// slots' values enter only the corner and the other rows >= p.  The slot itself matters: the augmented rows may
// straddle a 16-row block edge and then take another, equally accurate, route.
//
// GROUPED (lsspa_multi_lift_set_players): the players are groups of columns.  The orderings are then explicit rows -- the
// host's expansions of the group orderings, baseline first, rows 2 s and 2 s + 1 the two of an antithetical sample -- and a
// slot does not end with p lifts in HBM: they go to an LDS vector indexed by COLUMN, and one thread a group k < g adds its
// columns cols[off[k] .. off[k+1]) in ascending order from 0.0 (k_players.hip's fold and its order: plain adds, one thread
// a group) into out[sample][r][k].  Everything up to that epilogue is the column kernel's, line for line, so a group
// lift has the bits of that fold over the column kernel's lifts for the same row.  The GROUPED = false instantiation is
// the column kernel as it was.
//
// The second kernel folds a batch's lift vectors [B][m][p] into running (n, mean, M2) per entry: Welford over the batch
// in sample order, one Chan merge into the state (k_pairs.hip's scheme), a thread an entry, no atomics.
#include "kernels.h"
#include "tiles.h"

namespace lsspa {

namespace {

constexpr int RB = MLIFT_RB;
constexpr int VEC = 128;        // stride of a saved vector (p <= 104)

__device__ __forceinline__ int sw(int r, int c) { return r * 16 + (c ^ ((r >> 1) << 1)); }
__device__ __forceinline__ int tri_blk(int i, int j) { return i * (i + 1) / 2 + j; }   // i >= j

constexpr int SINV_LD = 17;

// One wave: factor the 16 x 16 diagonal block blk (swizzled, lower part valid) in place -- L below and on the
// diagonal, the strictly lower part of L^-1 mirrored above it -- and write its inverse to s_inv (16 x SINV_LD) and
// 1 / L[i][i] to s_rd[0..15] (k_small.hip: wave_factor16_sw).  tol: the pivot thresholds of the block's rows.
__device__ __forceinline__ void wave_factor16_sw(double* blk, double* s_inv, double* s_rd, const double* tol, int lane,
                                                 int& bad) {
  const int l15 = lane & 15, l4 = lane >> 4;
  d4 t, y;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = acc_row(l4, r);
    t[r] = (l15 <= row) ? blk[sw(row, l15)] : blk[sw(l15, row)];   // upper part: mirrored (what is stored there is ignored)
    y[r] = (row == l15) ? 1.0 : 0.0;
  }
  factor16_acc<double>(t, y, tol[l15], lane, bad);
  double dj;
  const bool holds = acc_diag<double>(t, l15, l4, dj);
  const double rs_mine = fast_rsqrt<double>(dj);                  // 1 / L[j][j]
  if (holds) s_rd[l15] = rs_mine;
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = acc_row(l4, r);
    const double rs_row = s_rd[row];
    const double xv = (l15 <= row) ? y[r] * rs_row : 0.0;         // (L^-1)[row][l15]
    if (l15 >= row) blk[sw(l15, row)] = t[r] * rs_row;
    s_inv[row * SINV_LD + l15] = xv;
    if (l15 < row) blk[sw(l15, row)] = xv;                        // the strictly lower part of L^-1, mirrored
  }
}

// element (m, k) of the inverse of a factored diagonal block
__device__ __forceinline__ double inv_elem(const double* blk, const double* rd, int m, int k) {
  const double off = blk[sw(min(m, k), max(m, k))];
  return (k < m) ? off : (k == m ? rd[m] : 0.0);
}

// T[q] -= A[q] B[q]^T on up to NT tiles at once, the tiles as element OFFSETS into M (k_small.hip: trailing_tiles; an
// array of pointers loses the LDS address space)
template <int NT>
__device__ __forceinline__ void trailing_tiles(double* M, const int (&To)[NT], const int (&Ao)[NT], const int (&Bo)[NT],
                                               int n, int l15, int l4) {
  double av[NT][4], bv[NT][4], tv[NT][4];
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int qq = (q < n) ? q : 0;        // a short batch re-reads tile 0 (uniform; nothing of it is stored)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      av[q][kk] = M[Ao[qq] + sw(l15, 4 * kk + l4)];
      bv[q][kk] = M[Bo[qq] + sw(l15, 4 * kk + l4)];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) tv[q][r] = M[To[qq] + sw(acc_row(l4, r), l15)];
  }
  d4 o[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) o[q] = d4_zero();
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int q = 0; q < NT; ++q) o[q] = mfma(av[q][kk], bv[q][kk], o[q]);
#pragma unroll
  for (int q = 0; q < NT; ++q)
    if (q < n) {
#pragma unroll
      for (int r = 0; r < 4; ++r) M[To[q] + sw(acc_row(l4, r), l15)] = tv[q][r] - o[q][r];
    }
}

constexpr int MAXNB = (MLIFT_MAX_P + RB) / 16;     // 7

}  // namespace

template <bool GROUPED>
__global__ __launch_bounds__(512) void multi_lift_kernel(MultiLiftArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int nb = a.nb, p = a.p;
  const int ntri = nb * (nb + 1) / 2;
  double* const M0 = smem;                     // training matrix -> L -> lift terms
  double* const M1 = M0 + ntri * 256;          // test matrix -> L_t -> V
  double* const s_inv = M1 + ntri * 256;       // [2][16 * SINV_LD]: inverse of the current diagonal block
  double* const s_rdb = s_inv + 2 * 16 * SINV_LD;   // [2][128]: 1 / L[i][i]
  double* const s_tol = s_rdb + 256;           // [2][128]: pivot thresholds (rows >= p: zero)
  double* const s_z = s_tol + 256;             // [RB][VEC]
  double* const s_y = s_z + RB * VEC;          // [RB][VEC]
  int32_t* const s_perm = reinterpret_cast<int32_t*>(s_y + RB * VEC);   // [128]
  // GROUPED: a slot's lifts by column [VEC], then the player map's CSR off [g + 1] and cols [p - n_base], 128 words each
  double* const s_lift = reinterpret_cast<double*>(s_perm + 128);
  int32_t* const s_off = reinterpret_cast<int32_t*>(s_lift + VEC);
  int32_t* const s_cols = s_off + 128;
  __shared__ int s_bad;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = wv >> 2, w = wv & 3, t2 = tid & 255;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int ord = blockIdx.x;
  const int r0 = blockIdx.y * RB;                       // the chunk's first response
  const int cnt = min(RB, a.count - r0);                // live slots (>= 1 by the grid)
  const int sample = ord / a.per_sample;
  // GROUPED: every ordering is a row of its own; else the pair's second ordering is the first read backwards
  const int32_t* perm = a.perms + (int64_t)(GROUPED ? ord : sample) * p;
  const bool backwards = !GROUPED && a.per_sample == 2 && (ord & 1);

  if (tid < 128) s_perm[tid] = (tid < p) ? perm[backwards ? p - 1 - tid : tid] : 0;
  if constexpr (GROUPED) {
    if (tid >= 128 && tid < 256) s_off[tid - 128] = (tid - 128 <= a.ng) ? a.off[tid - 128] : 0;
    if (tid >= 256 && tid < 384) s_cols[tid - 256] = (tid - 256 < a.n_cols) ? a.cols[tid - 256] : 0;
  }
  if (tid == 0) s_bad = 0;
  __syncthreads();

  // ---- permuted gather of both matrices (lower blocks), augmented rows p .. p + cnt - 1, identity below ------------
  {
    double* const M = half ? M1 : M0;
    const double* __restrict__ S = half ? a.H : a.G;
    const double* __restrict__ sv = (half ? a.h : a.g) + (int64_t)r0 * p;
    const double aug = a.aug[half];
    const int r = t2 >> 4, c = t2 & 15;
    const int swrc = sw(r, c);
    // a thread's rows are r, r + 16, ..: exactly one of them, ia, lies in p .. p + 15
    const int slot = (r - p) & 15, ia = p + slot;
    const bool live = slot < cnt;
    int pr[MAXNB], pc[MAXNB];
#pragma unroll
    for (int b = 0; b < MAXNB; ++b) {
      pr[b] = s_perm[min(16 * b + r, p - 1)];
      pc[b] = s_perm[min(16 * b + c, p - 1)];
    }
    double gv[MAXNB * (MAXNB + 1) / 2], av[MAXNB];
#pragma unroll
    for (int bi = 0; bi < MAXNB; ++bi)
#pragma unroll
      for (int bj = 0; bj <= bi; ++bj)
        if (bi < nb) gv[bi * (bi + 1) / 2 + bj] = S[(int64_t)pr[bi] * a.ld + pc[bj]];
#pragma unroll
    for (int bj = 0; bj < MAXNB; ++bj) av[bj] = (bj < nb && live) ? sv[(int64_t)slot * p + pc[bj]] : 0.0;
#pragma unroll
    for (int bi = 0; bi < MAXNB; ++bi)
#pragma unroll
      for (int bj = 0; bj <= bi; ++bj)
        if (bi < nb) {
          const int i = 16 * bi + r, j = 16 * bj + c;
          double v;
          if (i < p) v = (j <= i) ? gv[bi * (bi + 1) / 2 + bj] : 0.0;
          else if (i == ia && live) v = (j < p) ? av[bj] : (j == i ? aug : 0.0);
          else v = (i == j) ? 1.0 : 0.0;
          M[(bi * (bi + 1) / 2 + bj) * 256 + swrc] = v;
        }
    if (t2 < 128) {
      const int i = t2;
      s_tol[half * 128 + i] = (i < p) ? a.piv_tol * S[(int64_t)s_perm[i] * a.ld + s_perm[i]] : 0.0;
    }
  }
  __syncthreads();

  // ---- blocked Cholesky of both matrices at once (right-looking, 16 x 16 blocks; k_small.hip) ----------------------
  {
    double* const M = half ? M1 : M0;
    double* const inv = s_inv + half * 16 * SINV_LD;
    double* const rd = s_rdb + half * 128;
    const double* const tol = s_tol + half * 128;
    int bad = 0;
    const int fw = half;       // the factoring wave: wave 0 of the training half, wave 1 of the test half
    if (w == fw) wave_factor16_sw(M, inv, rd, tol, lane, bad);
    if (w == fw) __builtin_amdgcn_s_setprio(3);
    __syncthreads();
    for (int kb = 0; kb < nb; ++kb) {
      // panel: L[ib][kb] = T[ib][kb] Ld^-T, in place
      for (int ib = kb + 1 + w; ib < nb; ib += 4) {
        double* const Tb = M + tri_blk(ib, kb) * 256;
        d4 o = d4_zero();
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int kx = 4 * kk + l4;
          o = mfma(Tb[sw(l15, kx)], inv[l15 * SINV_LD + kx], o);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) Tb[sw(acc_row(l4, r), l15)] = o[r];
      }
      __syncthreads();
      if (kb + 1 == nb) break;
      // trailing update with look-ahead: the factoring wave takes the next diagonal tile alone and factors it at once
      if (w == fw) {
        const int To[1] = {tri_blk(kb + 1, kb + 1) * 256}, Ao[1] = {tri_blk(kb + 1, kb) * 256};
        trailing_tiles<1>(M, To, Ao, Ao, 1, l15, l4);
        __builtin_amdgcn_wave_barrier();
        wave_factor16_sw(M + To[0], inv, rd + 16 * (kb + 1), tol + 16 * (kb + 1), lane, bad);
      } else {
        const int me = (w + 3 - fw) % 4;          // 0, 1, 2 among the three helpers
        int To[4], Ao[4], Bo[4];
        int have = 0, tcount = 0;
        for (int ib = kb + 2; ib < nb; ++ib)
          for (int jb = kb + 1; jb <= ib; ++jb) {
            if ((tcount++ % 3) != me) continue;
            To[have] = tri_blk(ib, jb) * 256;
            Ao[have] = tri_blk(ib, kb) * 256;
            Bo[have] = tri_blk(jb, kb) * 256;
            if (++have == 4) {
              trailing_tiles<4>(M, To, Ao, Bo, 4, l15, l4);
              have = 0;
            }
          }
        if (have) trailing_tiles<4>(M, To, Ao, Bo, have, l15, l4);
      }
      __syncthreads();
    }
    if (w == fw) __builtin_amdgcn_s_setprio(0);
    if (bad && lane == 0) s_bad = 1;
  }

  // ---- z_s = row p + s of L, y~_s = row p + s of L_t (V overwrites L_t, the lift terms L) -------------------------
  for (int e = tid; e < RB * VEC; e += 512) {
    const int s = e / VEC, j = e % VEC;
    const int i = p + s;
    const bool in = j < p && s < cnt;
    const int off = in ? tri_blk(i >> 4, j >> 4) * 256 + sw(i & 15, j & 15) : 0;
    s_z[e] = in ? M0[off] : 0.0;
    s_y[e] = in ? M1[off] : 0.0;
  }
  __syncthreads();

  // ---- V = L^-1 L_t: wave cb solves the 16-column block cb, top down, in place of L_t; the solved blocks stay in the
  // wave's registers as the B operands of the rows below (k_small.hip) ------------------------------------------------
  if (wv < nb) {
    const int cb = wv;
    d4 vreg[MAXNB];
#pragma unroll
    for (int ii = 0; ii < MAXNB; ++ii) {        // row block i = cb + ii
      const int i = cb + ii;
      if (i >= nb) break;                        // uniform
      double af[MAXNB - 1][4];                   // fragments of L[i][cb + kk2], kk2 < ii
#pragma unroll
      for (int kk2 = 0; kk2 < MAXNB - 1; ++kk2)
        if (kk2 < ii) {
          const double* const Ab = M0 + tri_blk(i, cb + kk2) * 256;
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) af[kk2][kk] = Ab[sw(l15, 4 * kk + l4)];
        }
      double* const Tb = M1 + tri_blk(i, cb) * 256;
      double t[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) t[r] = Tb[sw(acc_row(l4, r), l15)];
      const double* const Ld = M0 + tri_blk(i, i) * 256;
      const double* const rd = s_rdb + 16 * i;
      double ie[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) ie[r] = inv_elem(Ld, rd, l15, 4 * r + l4);
      d4 acc = d4_zero();
#pragma unroll
      for (int kk2 = 0; kk2 < MAXNB - 1; ++kk2)
        if (kk2 < ii) {
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) acc = mfma(af[kk2][kk], vreg[kk2][kk], acc);
        }
#pragma unroll
      for (int r = 0; r < 4; ++r) t[r] -= acc[r];
      if (ii == 0) {   // L_t's diagonal block is lower triangular; its upper positions hold other data by now
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (l15 > acc_row(l4, r)) t[r] = 0.0;
      }
      d4 x = d4_zero();
#pragma unroll
      for (int r = 0; r < 4; ++r) x = mfma(ie[r], t[r], x);
      vreg[ii] = x;
#pragma unroll
      for (int r = 0; r < 4; ++r) Tb[sw(acc_row(l4, r), l15)] = x[r];
    }
  }
  __syncthreads();

  // ---- per response, in slot order: the lift terms  w[j][c] = V[j][c] (2 y~_c - N_j - N_{j-1}),  N_j = sum_{k <= j}
  // z_k V[k][c]  down column c (four threads a column, each a quarter of the rows; k_small.hip), into the dead storage
  // of L; then  lift_j = z_j / ||y||^2 * sum_{c <= j} w[j][c], four threads a row.  Only rows and columns < p are read.
  for (int s = 0; s < cnt; ++s) {
    const double* const z = s_z + s * VEC;
    const double* const yt = s_y + s * VEC;
    {
      const int c = tid >> 2, sq = tid & 3;
      const int cbk = c >> 4, cc = c & 15;
      const int len = (c < p) ? p - c : 0, per = (len + 3) >> 2;
      const int j0 = c + min(sq * per, len), j1 = c + min((sq + 1) * per, len);
      double part = 0.0;
      for (int j = j0; j < j1; ++j) part = fma(z[j], M1[tri_blk(j >> 4, cbk) * 256 + sw(j & 15, cc)], part);
      const double p1 = __shfl_up(part, 1, 4), p2 = __shfl_up(part, 2, 4), p3 = __shfl_up(part, 3, 4);
      double N = (sq >= 1 ? p1 : 0.0) + (sq >= 2 ? p2 : 0.0) + (sq >= 3 ? p3 : 0.0);
      const double y2 = 2.0 * yt[c];
      for (int j = j0; j < j1; ++j) {
        const int off = tri_blk(j >> 4, cbk) * 256 + sw(j & 15, cc);
        const double v = M1[off];
        const double Nn = fma(z[j], v, N);
        M0[off] = v * (y2 - Nn - N);
        N = Nn;
      }
    }
    __syncthreads();
    {
      const int j = tid >> 2, q = tid & 3;
      double sacc = 0.0;
      if (j < p)
        for (int c = q; c <= j; c += 4) sacc += M0[tri_blk(j >> 4, c >> 4) * 256 + sw(j & 15, c & 15)];
      sacc += __shfl_xor(sacc, 1);
      sacc += __shfl_xor(sacc, 2);
      if (j < p && q == 0) {
        const double lift = z[j] * sacc / a.yy[r0 + s];
        if constexpr (GROUPED) {
          s_lift[s_perm[j]] = lift;
        } else {
          double* dst = a.lifts + ((int64_t)sample * a.m + (r0 + s)) * p + s_perm[j];
          if (a.per_sample == 2) atomicAdd(dst, 0.5 * lift);   // the pair's two terms commute: order-independent sum
          else *dst = lift;
        }
      }
    }
    __syncthreads();           // the terms' storage is the next response's
    if constexpr (GROUPED) {
      // the fold, group k on thread 511 - k: the threads at the top end have no row or column of the scan (4 p <= 416),
      // so the next slot's terms start beside it.  The next slot writes s_lift only behind its own barrier, which these
      // threads reach after their reads.
      for (int k = 511 - tid; k < a.ng; k += 512) {
        double acc = 0.0;
        const int c1 = s_off[k + 1];
#pragma unroll 4
        for (int c = s_off[k]; c < c1; ++c) acc += s_lift[s_cols[c]];
        double* dst = a.lifts + ((int64_t)sample * a.m + (r0 + s)) * a.ng + k;
        if (a.per_sample == 2) atomicAdd(dst, 0.5 * acc);    // 0.5 x is exact and two addends commute: 0.5 (a + b)
        else *dst = acc;
      }
    }
  }
  if (tid == 0 && s_bad) atomicOr(a.info, 1);
}

// (n, mean, M2) per entry e < entries of the lift vectors [n_b][entries]: Welford over the batch in sample order, one Chan
// merge into the state that holds n_old samples
__global__ __launch_bounds__(256) void multi_lift_stats_kernel(const double* __restrict__ lifts, int64_t entries, int n_b,
                                                               double n_old, double* __restrict__ mean,
                                                               double* __restrict__ M2) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  double mb = 0.0, qb = 0.0;
  for (int s = 0; s < n_b; ++s) {
    const double x = lifts[(int64_t)s * entries + e];
    const double dl = x - mb;
    mb += dl / (double)(s + 1);
    qb += dl * (x - mb);
  }
  if (n_old == 0.0) {
    mean[e] = mb;
    M2[e] = qb;
  } else {
    const double nbd = (double)n_b, n = n_old + nbd;
    const double dl = mb - mean[e];
    mean[e] += dl * (nbd / n);
    M2[e] += qb + dl * dl * (n_old * nbd / n);
  }
}

size_t multi_lift_lds_bytes(int nb, bool grouped) {
  const size_t ntri = (size_t)nb * (nb + 1) / 2;
  return (2 * ntri * 256 + 2 * 16 * SINV_LD + 256 + 256 + 2 * RB * VEC) * sizeof(double) + 128 * sizeof(int32_t) +
         (grouped ? VEC * sizeof(double) + 2 * 128 * sizeof(int32_t) : 0);
}

hipError_t launch_multi_lift(const MultiLiftArgs& a, hipStream_t st) {
  const int64_t chunks = ((int64_t)a.count + RB - 1) / RB;
  if (a.p < 1 || a.p > MLIFT_MAX_P || a.nb != (a.p + RB + 15) / 16 || a.nb > MAXNB || a.n_samples < 1 || a.count < 1 ||
      a.m < a.count || (a.per_sample != 1 && a.per_sample != 2) || chunks > 65535 || a.ld < a.p || !a.G || !a.H || !a.g ||
      !a.h || !a.yy || !a.perms || !a.lifts || !a.info)
    return hipErrorInvalidValue;
  const bool grouped = a.ng != 0;
  // (off and cols are the library's own tables: player_map_build has checked that every column index is in 0 .. p-1)
  if (grouped && (a.ng < 1 || a.ng > a.p || a.n_cols < a.ng || a.n_cols > a.p || !a.off || !a.cols))
    return hipErrorInvalidValue;
  const size_t bytes = multi_lift_lds_bytes(a.nb, grouped);
  if (bytes > LDS_BYTES_PER_CU) return hipErrorInvalidValue;
  const dim3 grid(a.n_samples * a.per_sample, (unsigned)chunks);
  if (grouped) {
    static DynLdsGrant grant;   // per device
    hipError_t e = grant.ensure(reinterpret_cast<const void*>(multi_lift_kernel<true>), bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(multi_lift_kernel<true>, grid, dim3(512), bytes, st, a);
  } else {
    static DynLdsGrant grant;   // per device
    hipError_t e = grant.ensure(reinterpret_cast<const void*>(multi_lift_kernel<false>), bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(multi_lift_kernel<false>, grid, dim3(512), bytes, st, a);
  }
  return hipGetLastError();
}

hipError_t launch_multi_lift_stats(const double* lifts, int64_t entries, int n_b, int64_t n_old, double* mean, double* M2,
                                   hipStream_t st) {
  if (!lifts || !mean || !M2 || entries < 1 || n_b < 1 || n_old < 0 || (entries + 255) / 256 > 0x7fffffffll)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(multi_lift_stats_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, lifts, entries,
                     n_b, (double)n_old, mean, M2);
  return hipGetLastError();
}

}  // namespace lsspa
