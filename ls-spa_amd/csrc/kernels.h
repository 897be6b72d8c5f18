// Host-side launchers of the LS-SPA HIP kernels.  Every launcher checks its shape
// assumptions before launching (a faulting kernel can take the whole node down).
//
// The per-ordering kernels exist in two element types: fp64 (default; parity with the reference
// to ~1e-15) and fp32 (work matrices, factors and V in float; Gram reduction, lift accumulation and
// running statistics stay fp64).  `f32 != 0` selects the fp32 instantiation; the `void*` work
// buffers then hold floats.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "boot_plan.h"
#include "players.h"

namespace lsspa {

// Dynamic LDS beyond the 64 KB default needs hipFuncAttributeMaxDynamicSharedMemorySize, which is set on the CURRENT
// device's copy of the function: remember the size granted per device (a second engine on another GPU of the same
// process must set it again), under a lock (two engines may launch from two host threads).
struct DynLdsGrant {
  static constexpr int MAX_DEVICES = 64;
  std::mutex mu;
  size_t granted[MAX_DEVICES] = {0};
  hipError_t ensure(const void* fn, size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    if (dev >= 0 && dev < MAX_DEVICES && granted[dev] >= bytes) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess && dev >= 0 && dev < MAX_DEVICES) granted[dev] = bytes;
    return e;
  }
};
constexpr size_t LDS_BYTES_PER_CU = 160 * 1024;   // gfx950

struct GatherArgs {
  const double* S[2];      // source Gram matrices (train, test), fp64, row-major, stride ld_src
  const float* Sf[2];      // optional fp32 copies of S (same stride): read instead of S when the work matrices are
                           // fp32 -- same values after rounding, half the source traffic
  const double* s[2];      // source right-hand sides (g, h)
  double aug[2];           // diagonal value of the augmented row
  int64_t ld_src;
  const int32_t* perms;    // [n_ord][p]
  int p, p_pad, n_ord, n_src;  // n_src = 1 (train only) or 2
  void* A;                 // [n_src * n_ord] chunk-major p_pad x p_pad matrices, lower triangles written
  double* diag0;           // [n_src * n_ord][p_pad]: the permuted diagonals before any update (pivot scale)
  int f32;
  int paired;              // orderings 2 s and 2 s + 1 are each other's reverse (antithetical pairs): one pass over
                           // the source rows writes both matrices
};
hipError_t launch_gather(const GatherArgs& a, hipStream_t st);
int max_features();   // largest p the per-ordering kernels take (32-bit element counts of one work matrix)
// dst[i] = (float)src[i]
hipError_t launch_to_f32(const double* src, float* dst, int64_t count, hipStream_t st);

// Fused small-p path (k_small.hip): one workgroup per ordering, gather -> two Choleskys -> V -> lifts in LDS.
// fp64, tri mode, p + 1 <= 128.  With per_sample == 2 orderings 2 s and 2 s + 1 each add half their lift vector
// to sample s (lifts must be zero beforehand); with 1 the lift vector is stored.
struct SmallArgs {
  const double* S[2];      // source Gram matrices (train, test), row-major, stride ld_src
  const double* s[2];      // source right-hand sides (g, h)
  double aug[2];           // diagonal value of the augmented row
  int64_t ld_src;
  const int32_t* perms;    // [n_ord][p]; with fwd_only [n_ord / 2][p]: ordering 2 s + 1 is sample s's read backwards
  int fwd_only;            // (per_sample == 2 only) the host stages and uploads half as much
  int p, nb, n_ord, per_sample;   // nb = ceil((p + 1) / 16)
  double* lifts;           // [n_ord / per_sample][p]
  double y_norm_sq;
  double piv_tol;
  int32_t* info;
  int variant;             // 0: the register-resident kernel where it applies (nb <= 7); 1: the LDS-resident kernel
  // the register-resident kernel checks every ordering's sum of lifts against the full model's R^2 itself (sum_tol >= 0;
  // off: -1): LSSPA_INFO_SUM into info[0] beyond sum_tol, the largest deviation above sum_quiet into info[2..3]
  double r2, sum_tol, sum_quiet;
};
bool small_p_checks_sum(const SmallArgs& a);
// One ordering through `folds` different reduced problems in one launch (lsspa_cv_lift_batch): grid (n_ord, folds), the
// kernel form launch_small_p picks for nb (register-resident for nb <= 7, LDS-resident for eight block rows).  Fold
// f = blockIdx.y has its problem behind the launch's at one stride -- S[.] + f mat, s[.] + f vec, the augmented rows'
// diagonals aug[2 f + .] (SmallArgs::aug is not read), 1 / ||y||^2 = inv_yy[f], its pivot flag in info[f].  Ordering o of
// fold f stores its p lifts, multiplied by inv_yy[f], to lifts[(o folds + f) p + .] by plain stores (per_sample and
// fwd_only only say how perms is read: with fwd_only ordering 2 s + 1 is row s read backwards); no atomics, no sum check;
// y_norm_sq, r2 and sum_* are not read.  ld_src is even and >= p + 1, mat even, the matrices 16-byte aligned;
// n_ord folds <= SMALL_FOLDS_MAX_GRID.  The fold arguments are a kernel parameter of their own: the one-problem
// kernels' arguments, and with them their code, stay what they were.
struct SmallFolds {
  int64_t mat, vec;
  const double* aug;       // [folds][2]
  const double* inv_yy;    // [folds]
  int folds;
};
constexpr int64_t SMALL_FOLDS_MAX_GRID = 1 << 16;
hipError_t launch_small_folds(const SmallArgs& a, const SmallFolds& fo, hipStream_t st);
size_t small_folds_lds_bytes(int nb);   // dynamic LDS of a workgroup of launch_small_folds
// Many problems on one set of orderings (lsspa_boot_lift_run): launch_small_folds' kernels and arguments with
// 1 <= fo.folds <= 65535 problems and n_ord fo.folds <= SMALL_FOLDS_MAX_GRID; problem blockIdx.y has its pivot flag in
// info[blockIdx.y].  No kernel of its own: the instantiations are launch_small_folds', whose refusals stay as they are.
hipError_t launch_small_problems(const SmallArgs& a, const SmallFolds& fo, hipStream_t st);
// host_perms.cpp: every row of perms [B][p] a permutation of 0..p-1?  (sets by AVX2 for 8 <= p <= 128, stamps otherwise;
// _plain: the stamp loop alone, the test's comparison)
bool all_permutations(const int32_t* perms, int B, int p, std::vector<int32_t>& mark);
bool all_permutations_plain(const int32_t* perms, int B, int p, std::vector<int32_t>& mark);
// host_perms.cpp: out [B][p] = argsort of the rows of keys [B][p] on up to `threads` native threads; redo [B] = 1 for the
// rows left to the caller (equal keys or a NaN: numpy's order there is its own); returns their number
int64_t argsort_rows_host(const double* keys, int64_t B, int p, int32_t* out, uint8_t* redo, int threads);
// host_perms.cpp: the 'argsort' ordering source as a native thread (Sobol' points by SciPy's recurrence + row argsort)
struct SobolSampler;
SobolSampler* sobol_sampler_create(int p, int bits, const uint64_t* sv_pb, const uint64_t* q0, double scale, int64_t limit,
                                   int block, int64_t ahead, int64_t ahead_unasked, int threads, int rank, int world);
void sobol_sampler_destroy(SobolSampler* s);
int sobol_sampler_take(SobolSampler* s, int64_t count, int32_t* out, int64_t cap, int64_t* n_taken, int64_t* n_own,
                       int64_t* redo_pos, int64_t* redo_id, int64_t* n_redo, const char** err);
bool small_p_eligible(int p);
size_t small_p_lds_bytes(int nb);
hipError_t launch_small_p(const SmallArgs& a, hipStream_t st);

// Blocked Cholesky, 128-wide panels (p_pad a multiple of 128).  diag0 / piv_tol: a pivot d counts as non-positive
// (LSSPA_INFO_NOT_PD) when d <= piv_tol * diag0.  One diagonal launch (block 0), then panel steps Jo = 0 ..
// p_pad/128 - 2: step Jo computes L[I, Jo] for the tiles below and its tile-0 workgroups update and factor diagonal
// block Jo + 1.
hipError_t launch_chol2_diag(void* A, void* Dinv, const double* diag0, double piv_tol, int32_t* info, int p_pad,
                             int n_mats, int f32, hipStream_t st,
                             int32_t* row_flags = nullptr);
// p_live: rows at or beyond it are identity padding (p + 1 rounded up to 16; 0 = none known): their all-zero
// accumulator tiles are left out of the products.
// X != null (tri mode): the matrices are [n_ord training][n_ord test] and step Jo also computes block column Jo of
// X = V^T = L_t^T L^-T ([n_ord] chunk-major p_pad x p_pad matrices, upper block triangle written) as extra tiles of
// the training factorisation; there is then one more step, Jo = p_pad/128 - 1, with X tiles only.
// pl (with X tiles): the lift scan of V^T is done by the X tiles themselves, block by block, before the block leaves
// the chip -- the lift kernel's pass over V^T falls away (launch_lift with fused = 1 only finishes).  flags must be
// zero before launch 0 of a batch; mode 2 also leaves the last panel's V^T unstored (nobody reads it then).
struct PanelLift {
  int32_t* flags;          // [n_mats]
  double* run;             // [n_ord][p_pad]
  double* Ppart;           // [n_ord][pstride], row block I' of V^T at [I' * p_pad]
  int64_t pstride;
  int p;                   // features
  int mode;                // 0 off, 1 scan, 2 scan + last panel of V^T not stored
};
// What launch_chol2_panel decides per launch, as a host function of its own (the tests read it through
// lsspa_debug_panel_plan): n_lt L tiles per matrix and n_x X tiles per ordering (has_X: X tiles are computed), n_ord as
// the kernel counts orderings (n_mats without X tiles), p_live clamped to p_pad, the 1-D grid, grouped (the workgroup
// -> (matrix, tile) map that walks eight matrices at a time) and xlast (the instantiation that leaves the last
// panel's dead columns out).  false: launch_chol2_panel refuses these arguments.
struct PanelPlan {
  int n_lt, n_x, n_ord, p_live, grouped, xlast;
  int64_t grid;
};
bool panel_plan(int p_pad, int Jo, int n_mats, int n_ord, bool has_X, int p_live, PanelPlan* out);
hipError_t launch_chol2_panel(void* A, void* Dinv, const double* diag0, double piv_tol, int32_t* info, int p_pad,
                              int Jo, int n_mats, int f32, hipStream_t st, int flags = 0, int p_live = 0,
                              void* X = nullptr, int n_ord = 0, const PanelLift* pl = nullptr);

struct StripArgs {
  const void* A;           // factored train matrices
  const void* Dinv;        // [n_mats][nblk][64][64]; the first n_ord entries belong to A
  const void* rhs;         // tri: factored test matrices (same layout as A); rect: unused
  const double* Ft;        // rect: transposed test factor [p][m_pad], fp64
  const int32_t* perms;    // rect only
  void* V;                 // [n_ord][v_rows][m_pad + 32]
  int p, p_pad, m_pad, n_ord, tri;
  int flags;               // developer A/B switches
  int f32;
  int row_live = 0;        // rows at or beyond it are identity padding of L (p + 1 rounded up to 16; 0 = unknown)
  int col_live = 0;        // columns at or beyond it are zero columns of the right-hand side (0 = unknown)
};
hipError_t launch_strip(const StripArgs& a, hipStream_t st);

struct LiftArgs {
  const void* A;           // factored train matrices (row p holds z)
  const void* At;          // tri: factored test matrices (row p holds y-tilde); rect: null
  const double* ytil;      // rect: [m_pad]
  const void* V;           // vt == 0: V row-major [v_rows][m_pad + 32]; vt != 0: V^T chunk-major p_pad x p_pad (tri)
  int vt = 0;
  const int32_t* perms;    // [n_ord][p]
  double* Ppart;           // [n_ord][m_pad/64][p_pad]
  double* lifts;           // [n_samples][p]
  double y_norm_sq;
  int p, p_pad, m_pad, n_ord, per_sample, tri;  // per_sample = 1 or 2 orderings per sample
  int f32;
  int paired;              // per_sample == 2 and ordering 2 s + 1 is ordering 2 s reversed
  int fused = 0;           // vt: Ppart already holds the X tiles' own sums, one row per 128-row block of V^T (PanelLift)
};
hipError_t launch_lift(const LiftArgs& a, hipStream_t st);
// |sum of a sample's lifts - r2| <= tol for every sample, else bit 8 (LSSPA_INFO_SUM) of info[0]; the largest deviation
// of all launches since the last reset as a double in info[2..3]
hipError_t launch_sum_check(const double* lifts, int n_samples, int p, double r2, double tol, int32_t* info,
                            hipStream_t st);

// Sampled attribution over groups of columns (lsspa_set_players): PlayerMap, the host side of the map, and its two host
// functions are declared in players.h.
// k_players.hip: out[s][k] = mean over the sample's `per` (1 or 2) rows of the sum of lifts[row][j] over group k's columns
// (off [g + 1], cols: PlayerMap's CSR on the device); lifts [n_samples * per][p], out [n_samples][g].  Fixed summation order.
hipError_t launch_fold_players(const double* lifts, int p, int per, const int32_t* off, const int32_t* cols, int g,
                               int n_samples, double* out, hipStream_t st);

// Sampled pairwise interaction index (lsspa_pairs_batch, k_pairs.hip).  lifts [3 n_samples][ld]: rows 3 s .. 3 s + 2 are
// the lift vectors of sample s's three orderings (expand_pair_rows, players.h), perms [n_samples][d] its orderings pi_s.
// Three launches: delta [n_samples][d] and pos [n_samples][d] (the inverse orderings) are written; every pair adjacent
// in an ordering folds its Delta into the tables t_count / t_mean / t_m2 [d][d] (kept at [a][b], a < b: Welford over the
// batch in sample order, one Chan merge into the table); phi [d] += the 3 n_samples rows, in order.
constexpr int PAIRS_MAX_D = 4096;   // LSSPA_PAIRS_MAX_D: positions are 16-bit, three d x d tables
hipError_t launch_pairs(const double* lifts, int ld, const int32_t* perms, int d, int n_samples, double* delta,
                        int16_t* pos, int64_t* t_count, double* t_mean, double* t_m2, double* phi, hipStream_t st);

// pending-batch moments about the current running mean: buf = [n_b, S (p), Q (p x p)]
// parts: workspace of stats_batch_slices(n_samples, p) * (1 + p + p*p) doubles (or NULL: one slice)
int stats_batch_slices(int n_samples, int p);
// samples per slice when n_samples are cut into nz slices: whole 16-sample steps
int stats_batch_per_slice(int n_samples, int nz);
hipError_t launch_stats_batch(const double* lifts, const double* mean, double* buf, int n_samples, int p,
                              int accumulate, double* parts, hipStream_t st);
// single GPU, small p: batch moments AND merge in one launch (no pending buffer): reads (mean, state[0] = n), writes
// the advanced ones to (mean_out, state_out) -- the caller swaps the buffers -- and updates M2 in place
bool stats_small_fusable(int n_samples, int p);
// the same for up to 32 chunks of samples (first sample and count of each, in `lifts`), folded and merged one after the
// other in one launch; mean_snap [n][p] / n_snap [n] (may be null): mean and n after every chunk
struct StatsChunks {
  static constexpr int MAX = 32;
  int n;
  int first[MAX], count[MAX];
};
hipError_t launch_stats_small_multi(const double* lifts, const double* mean, const double* state, double* mean_out,
                                    double* state_out, double* M2, const StatsChunks& ch, int p, double* mean_snap,
                                    double* n_snap, hipStream_t st);
hipError_t launch_stats_small_fused(const double* lifts, const double* mean, const double* state, double* mean_out,
                                    double* state_out, double* M2, int n_samples, int p, hipStream_t st);
// Chan merge of the pending batch into (n, mean, M2); n lives in state[0] (state[1] is the fused kernel's ticket and
// must start at zero).  *cleared: the launch also zeroed the pending buffer (small p: one fused kernel)
hipError_t launch_stats_merge(double* buf, double* state_n, double* mean, double* M2, int p, hipStream_t st,
                              bool* cleared);

// upper-triangle packing of the pending-batch buffer for the all-reduce (Q is symmetric):
// packed = [n_b, S (p), Q[i][i..p-1] ...], stats_packed_count(p) = 1 + p + p (p + 1) / 2 elements
int64_t stats_packed_count(int p);
hipError_t launch_stats_pack(const double* buf, double* packed, int p, hipStream_t st);
hipError_t launch_stats_unpack(const double* packed, double* buf, int p, hipStream_t st);

// theta = L^-T z for the factor stored in A (identity ordering), single workgroup; theta is fp64
// wg: workspace of p doubles for p beyond what a CU's LDS holds (may be null below that)
hipError_t launch_backsolve(const void* A, double* theta, int p, int p_pad, int f32, hipStream_t st,
                            double* wg = nullptr);

// out[j] = L_jj^2 / G_jj of the factor stored in A (identity ordering; G [p][p_pad] row-major), j < p
hipError_t launch_rel_pivots(const void* A, const double* G, double* out, int p, int p_pad, int f32, hipStream_t st);

// Gram contraction  C = Z^T Z, Z = [X | y]  (rows n, P1 = p + 1 columns), fp64 MFMA, split over rows
struct GramArgs {
  const void* X;           // [n][ld] row-major (device)
  const void* y;           // [n]
  int64_t n, ld;
  int p;                   // features; Z has p + 1 columns
  int is_f32;              // element type of X / y
  double* slabs;           // workspace [n_split][n_pairs][128][128]
  int n_split;
  double* C;               // out: [P1pad][P1pad] full symmetric, P1pad = round_up(p + 1, 128)
  int accumulate;          // C += (row chunks of a streamed matrix) instead of C =
  int variant = 0;         // developer A/B switches (bit 0: workgroup id = unit, no XCD-contiguous map)
};
// What a launch is cut into (host and device agree on it through this struct).  Units come in three classes -- A:
// off-diagonal pairs of full tiles (16 blocks a wave and k-step), B: pairs whose tile i is the ragged last tile
// (2 xlive blocks), C: duos (18) -- each with its own slice count (gram_plan: 16 : 18 : 20 from six tiles on).
struct GramPlan {
  int nt;                 // 128-column tiles of Z = [X | y]
  int xlive;              // live 16-column blocks of the last tile
  int cnt[3];             // units per slice, classes A, B, C
  int slices[3];          // row slices per class
  int rps[3];             // rows per slice (multiple of 16)
  int per_xcd;            // workgroups per XCD (grid = 8 x per_xcd)
  int natural;            // developer A/B: unit = workgroup id (units of a slice spread over the XCDs)
  __host__ __device__ int total() const { return cnt[0] * slices[0] + cnt[1] * slices[1] + cnt[2] * slices[2]; }
};
// n_split = row slices of class A (gram_default_split for the launch's rows); launch_gram cuts its launch by it
GramPlan gram_plan(int64_t n, int p, int n_split, int variant = 0);
size_t gram_workspace_bytes(int p, int n_split);
int gram_default_split(int64_t n, int p);
hipError_t launch_gram(const GramArgs& a, hipStream_t st);
// G[a][b] = C[a][b] * scale + (a == b) * reg ; g[a] = C[p][a] * scale ; scalars[0] = C[p][p] * scale
hipError_t launch_gram_finalize(const double* C, int p, double scale, double reg, double* G, int64_t ldg,
                                double* g, double* scalar_out, hipStream_t st);

// Device-side error estimator.  launch_error_draws: draws[d][a] = sum_k Xi[d][k] (H[k][a] - mean[a]) * scale for
// the 1024 draws d (Xi [1024][ldxi], H [n_pad][ldh], both zero-padded to n_pad samples, n_pad a multiple of 16;
// ldh and ldd cover ceil(p/128)*128 columns).  launch_error_quantiles: out[a] = 0.95-quantile of |draws[:, a]|,
// out[p] = 0.95-quantile of the row 2-norms (norms [1024] is a workspace).
constexpr int ERR_DRAWS = 1024;
hipError_t launch_error_draws(const double* Xi, int ldxi, const double* H, int ldh, int n_pad,
                              const double* mean, double scale, int p, double* draws, int ldd, hipStream_t st);
// pack_mean / pack_n (optional): out is [2 p + 2] and also receives the running mean and n behind the p + 1 quantiles.
hipError_t launch_error_quantiles(const double* draws, int ldd, int p, double* norms, double* out,
                                  hipStream_t st, const double* pack_mean = nullptr, const double* pack_n = nullptr);
// the same on x = (D - s mean^T) * scale evaluated as it is read (one rank: no draws buffer); always packed
hipError_t launch_error_quantiles_running(const double* D, const double* s, const double* mean, double scale, int ld,
                                          int p, double* norms, double* out, const double* pack_n, hipStream_t st);
// Running form of the estimator (k_error.hip): Xi[d][k] = standard normal made by Philox4x32-10 from (seed, sample id
// first_id + k stride, draw d), k < count, zero up to n_pad (a multiple of 16).  launch_error_xi stores Xi [1024][n_pad]
// (also the test hook); launch_error_accumulate does that into the workspace Xi [1024][n_pad] and adds
// D[1024][ldh] += Xi L, s[1024] += Xi 1 for the chunk's lift vectors L; launch_error_running_draws:
// x = (D - s mean^T) * scale.
// the chunks of a group folded into the running estimator by launch_error_group, and the checks that belong to them
struct EstChunks {
  static constexpr int MAX = 32;
  int n;
  int first[MAX], count[MAX], n_pad[MAX];   // first sample in the lane's lift buffer, samples, samples padded to 16
  long long xi_off[MAX];                    // the chunk's normals in the workspace (doubles)
  long long first_id[MAX];                  // global sample number of the chunk's first sample
  double scale[MAX];                        // 1 / sqrt(n (n - 1)) of the chunk's check, 0 = no check
};
struct EstChecks {
  int n;
  int chunk[EstChunks::MAX], slot[EstChunks::MAX];
  double scale[EstChunks::MAX];
};
hipError_t launch_error_group(uint64_t seed, int64_t stride, const EstChunks& ch, const EstChecks& ck, double* Xi,
                              const double* lifts, int p, int ld, double* P, double* S, double* D, double* s,
                              double* Dsnap, double* ssnap, const double* mean_snap, const double* n_snap,
                              double* norms, double* res, hipStream_t st);
hipError_t launch_error_xi(uint64_t seed, int64_t first_id, int64_t stride, int count, int n_pad, double* Xi,
                           hipStream_t st);
// L: raw == 0: [n_pad][ldl = ldh], padded and zero-filled; raw != 0: [count][ldl >= p] as the lift kernels wrote it
hipError_t launch_error_accumulate(uint64_t seed, int64_t first_id, int64_t stride, int count, int n_pad, double* Xi,
                                   const double* L, int ldl, int raw, int ldh, int p, double* D, double* s,
                                   hipStream_t st);
hipError_t launch_error_running_draws(const double* D, const double* s, const double* mean, double scale, int p,
                                      int ld, double* draws, hipStream_t st);

// unit test hook: D = A(16x4) * B(4x16) on one wave through Tr<T>::mfma / acc_row (fp64 or fp32)
hipError_t launch_mfma_probe(const double* A, const double* B, double* D, int f32, hipStream_t st);

// Exact attribution by subset enumeration (k_subsets.hip), p <= SUBSETS_MAX_P, fp64.  Features 0 .. q-1 are the low
// ones (q = subsets_low_features(p)); high subset number hi is the set {q + j : bit j of hi}.  The enumeration runs
// `units` workgroups; unit u owns high subsets u per .. (u + 1) per - 1 (units * per = 2^(p - q)) and one launch takes
// steps s0 .. s1 - 1 of every unit, adding to the unit's row of part [units][p + 1]:
//   part[u][j] += sum over its subsets K containing j of (w(|K| - 1) + w(|K|)) v(K),  part[u][p] += sum w(|K|) v(K)
// with w = wa, wb below; phi_j = sum_u part[u][j] - sum_u part[u][p] (launch_subsets_reduce, fixed order).
// With inter (the pairwise interaction index, k_subsets.hip's header) a row is subsets_inter_cols(p) wide:
//   [0 .. p] as above | T0 | T1_i [p] | T2_ij [p (p - 1) / 2], pairs i < j row-major;  I_ij = T0 - T1_i - T1_j + T2_ij
// of the column sums, and w holds three more rows: gamma, beta + gamma, alpha + 2 beta + gamma by |K|.
constexpr int SUBSETS_MAX_P = 32;
struct SubsetArgs {
  const double* G;         // [p][ldg] training Gram
  const double* g;         // [p]
  const double* H;         // [p][ldh] test Gram
  const double* h;         // [p]
  int64_t ldg, ldh;
  const double* w;         // [2][SUBSETS_MAX_P + 1]: wa[k] = w(k - 1) (0 for k = 0), wb[k] = w(k) (0 for k = p);
                           // inter: [5][SUBSETS_MAX_P + 1], the interaction weights after them
  int p, q;
  double piv_tol;          // relative pivot test: a pivot d <= piv_tol G_jj raises LSSPA_INFO_NOT_PD
  const double* inv_yy;    // [replicates] 1 / ||y_test||^2 (device)
  uint64_t per;            // high subsets per unit
  double* part;            // [units][p + 1], inter: [units][subsets_inter_cols(p)]
  int32_t* info;           // [replicates] bit 1: a pivot failed
  // Replicates (the bootstrap, k_boot.hip): a launch with `reps` replicates runs them as its second grid dimension;
  // replicate r has its problem at the dense replicate stride behind the launch's: G + r p ldg, g + r p, H + r p ldh,
  // h + r p, inv_yy[r], info[r], part + r units cols (cols: the table's width, p + 1 or inter's).  One replicate (every
  // other launch): r = 0, nothing moves.
};
int subsets_low_features(int p);
int subsets_inter_cols(int p);
// reps > 1: the replicates behind the launch's problem (SubsetArgs) as its second grid dimension, phi-only or inter
hipError_t launch_subsets_enum(const SubsetArgs& a, uint64_t units, uint64_t s0, uint64_t s1, bool inter,
                               hipStream_t st, int reps = 1);
// out[j] = sum over the units of part[u][j], j < cols (the table's width), in a fixed order; replicate r of `reps` reads
// part + r units cols and writes out + r cols
hipError_t launch_subsets_reduce(const double* part, int64_t units, int cols, double* out, hipStream_t st,
                                 int reps = 1);
// Best subset of every size (lsspa_subsets_best): the units, steps and launches of launch_subsets_enum (reps = 1), but
// a.part [units][p + 1] holds each unit's largest v(K) per size |K| and bm [units][p + 1][2] its mask (bit j = feature
// j) and a found flag; both zeroed before the first launch, every launch merges into them.  Larger value wins, on equal
// values the smaller mask; only subsets K with (K & include) == include whose own pivots passed are candidates.  per
// must be at most 2^13 (it is for units = min(2^(p - q), 8192)).
// reps > 1 (1 <= reps <= 65535; lsspa_boot_best_run): the replicates behind the launch's problem as its second grid
// dimension -- G, g, H, h, inv_yy and info as launch_subsets_enum's, the tables [reps][units][p + 1] and
// [reps][units][p + 1][2].  A replicate's result does not depend on the launches' cut or on the replicates beside it.
hipError_t launch_subsets_best(const SubsetArgs& a, uint64_t units, uint64_t s0, uint64_t s1, uint32_t include,
                               uint32_t* bm, hipStream_t st, int reps = 1);
// out_v[k], out_m[k][2] (mask, found): the best of size k = 0 .. p over the units' rows; replicate r of `reps` reads its
// rows of the tables and writes out_v + r out_stride, out_m + 2 r out_stride (out_stride >= p + 1)
hipError_t launch_subsets_best_reduce(const double* bv, const uint32_t* bm, int64_t units, int p, double* out_v,
                                      uint32_t* out_m, hipStream_t st, int reps = 1, int64_t out_stride = 0);
// The T best subsets of every size (lsspa_subsets_top), 1 <= T <= SUBSETS_TOP_MAX: launch_subsets_best's units, steps,
// launches, candidates and order (one problem, no replicates), but a unit keeps per size a list of its T best so far,
// best first: a.part [units][p + 1][T] the values, tm [units][p + 1][T] the masks (bit j = feature j), tc [units][p + 1]
// how many entries of a list are valid.  tc is zeroed before the first launch (the entries need not be); every launch
// merges into the lists.  The order is strict (masks are unique), so the lists do not depend on the launches' cut.
constexpr int SUBSETS_TOP_MAX = 16;
hipError_t launch_subsets_top(const SubsetArgs& a, uint64_t units, uint64_t s0, uint64_t s1, uint32_t include, int T,
                              uint32_t* tm, int32_t* tc, hipStream_t st);
// out_v [p + 1][T], out_m [p + 1][T], out_c [p + 1]: per size k the T best over the units' lists in the same order and
// their number, min(T, candidates of size k); NaN and 0 past it.  units <= 8192.
hipError_t launch_subsets_top_reduce(const double* tv, const uint32_t* tm, const int32_t* tc, int64_t units, int p, int T,
                                     double* out_v, uint32_t* out_m, int32_t* out_c, hipStream_t st);
// K-fold cross-validation (lsspa_cv_*; k_cv.hip has the kernels before the enumeration).  The `folds` reduced problems
// lie behind a's at the dense replicate stride, as a launch's replicates do, with one info word each.
// launch_subsets_cv_best: launch_subsets_best's units, steps, launches, tables, candidates and order, for
//   v_cv(K) = v_0(K) + ... + v_{folds-1}(K), the fp64 sum in this order of the values launch_subsets_debug gives for
// the fold problems; a candidate's own pivots passed in every fold, and a failed pivot raises a.info[fold].
// launch_subsets_best_reduce takes the best over the units.  2 <= folds <= CV_MAX_FOLDS.
constexpr int CV_MAX_FOLDS = 32;
hipError_t launch_subsets_cv_best(const SubsetArgs& a, int folds, uint64_t units, uint64_t s0, uint64_t s1,
                                  uint32_t include, uint32_t* bm, hipStream_t st);
// vals[i] = v_cv(masks[i]) and, unless null, vfold[i][f] = v_f(masks[i]) by that kernel's own fold-step
hipError_t launch_subsets_cv_debug(const SubsetArgs& a, int folds, const uint64_t* masks, int64_t n, double* vals,
                                   double* vfold, hipStream_t st);
size_t subsets_cv_lds_bytes();     // static LDS of a workgroup of launch_subsets_cv_best
// launch_subsets_cv_top: launch_subsets_cv_best's units, steps, launches, fold-step, candidates (whose sum is also above
// -inf) and info words with launch_subsets_top's lists, order and tables: a.part [units][p + 1][T], tm [units][p + 1][T],
// tc [units][p + 1], tc zeroed before the first launch; launch_subsets_top_reduce merges the units' lists.
hipError_t launch_subsets_cv_top(const SubsetArgs& a, int folds, uint64_t units, uint64_t s0, uint64_t s1,
                                 uint32_t include, int T, uint32_t* tm, int32_t* tc, hipStream_t st);
size_t subsets_cv_top_lds_bytes(int T);   // LDS of a workgroup of launch_subsets_cv_top: static and the lists at this T
// wt[f][i] = 1.0 if fid[i] == f else 0.0, f < folds, i < n: the folds' indicator weights for launch_boot_gram
hipError_t launch_cv_weights(const int32_t* fid, int64_t n, int folds, double* wt, hipStream_t st);
// The fold problems from the per-fold Grams S [folds][c][c] (c = p + 1) and the folds' sizes nf [folds] of n rows:
//   G[f] = (sum_{j != f} S[j])[:p,:p] / (n - nf[f]) + reg I (j ascending), g[f] likewise from column p,
//   H[f] = S[f][:p,:p], h[f] = S[f][:p,p], inv_yy[f] = 1 / sum_j S[j][p][p] (j ascending, the same for every f)
// p <= GROUPS_MAX_P: the grouped calls (lsspa_cv_groups_*) read the same problems
hipError_t launch_cv_finalize(const double* S, const int32_t* nf, int64_t n, int p, int folds, double reg, double* G,
                              double* g, double* H, double* h, double* inv_yy, hipStream_t st);
// phi_fold[f][j] = out[f][j] - out[f][p] of the enumeration's column sums out [folds][p + 1], phi[j] = their sum over f
// in ascending order
hipError_t launch_cv_foldsum(const double* out, int p, int folds, double* phi_fold, double* phi, hipStream_t st);
// vals[i] = v(masks[i]) by the enumeration's own device code (test hook); masks < 2^p
hipError_t launch_subsets_debug(const SubsetArgs& a, const uint64_t* masks, int64_t n, double* vals, hipStream_t st);
// Hh = [H = Ft Ft^T (p x p, stride p) | h = Ft ytil] of a rect-mode test factor Ft [p][ldf], m columns used
// (p <= 64: the grouped enumeration of k_groups.hip uses it too)
hipError_t launch_subsets_test_gram(const double* Ft, int64_t ldf, const double* ytil, int p, int m, double* Hh,
                                    hipStream_t st);

// Exact attribution over groups of columns (k_groups.hip), g <= GROUPS_MAX_G groups, p <= GROUPS_MAX_P columns, fp64.
// groups_layout turns labels (-1: baseline, 0 .. g-1: group) into the kernels' layout: gl low groups (the smallest,
// ql <= GROUPS_LOW_COLS columns together) and gh high ones; gid[r] is the label of the layout's group r (low groups
// first).  tab: the columns in layout order (baseline, high groups, low groups), per column its high group (-1: none)
// and its place inside it, the high groups' sizes and per low column its low group.  High subset number hi is the set
// of high groups {j : bit j of hi}.  Units, steps and the partial table [units][g + 1] (layout numbering, then b) are
// those of launch_subsets_enum; launch_subsets_reduce sums the table.  With inter (the pairwise interaction index
// between groups, k_groups.hip's header) a row is subsets_inter_cols(g) wide, as launch_subsets_enum's with p = g and
// the layout's numbering, and w holds the three rows of interaction weights of g players.
constexpr int GROUPS_MAX_G = 32, GROUPS_MAX_P = 64, GROUPS_LOW_COLS = 6;
constexpr int GROUPS_TAB_COLS = 0, GROUPS_TAB_COLGRP = GROUPS_MAX_P, GROUPS_TAB_COLIN = 2 * GROUPS_MAX_P,
              GROUPS_TAB_HSIZE = 3 * GROUPS_MAX_P, GROUPS_TAB_LGRP = GROUPS_TAB_HSIZE + GROUPS_MAX_G,
              GROUPS_TAB_LEN = GROUPS_TAB_LGRP + 8;
// the two words behind the GROUPS_LOW_COLS of LGRP, 0 in every layout of groups_layout: the inner players of an Owen
// enumeration (launch_groups_owen) as masks over the layout's low groups (bits of the lane) and high groups (bits of hi)
constexpr int GROUPS_TAB_OWEN_LO = GROUPS_TAB_LGRP + GROUPS_LOW_COLS, GROUPS_TAB_OWEN_HI = GROUPS_TAB_OWEN_LO + 1;
static_assert(GROUPS_TAB_OWEN_HI < GROUPS_TAB_LEN, "the Owen masks live inside the layout table");
struct GroupLayout {
  int p, ng, nb, gl, gh, ql;
  int gid[GROUPS_MAX_G];
  int32_t tab[GROUPS_TAB_LEN];
};
// nullptr, or what is wrong with the labels
const char* groups_layout(const int32_t* labels, int p, int g, GroupLayout& L);
struct GroupArgs {
  const double* G;         // [p][ldg] training Gram
  const double* g;         // [p]
  const double* H;         // [p][ldh] test Gram (symmetric)
  const double* h;         // [p]
  int64_t ldg, ldh;
  const double* w;         // [2][GROUPS_MAX_G + 1]: wa[k] = w(k - 1) (0 for k = 0), wb[k] = w(k) (0 for k = g);
                           // inter: [5][GROUPS_MAX_G + 1], the interaction weights after them
  const int32_t* tab;      // GroupLayout::tab on the device
  int p, ng, nb, gl, gh, ql;
  double piv_tol;          // relative pivot test: a pivot d <= piv_tol G_jj raises LSSPA_INFO_NOT_PD
  double inv_yy;           // 1 / ||y_test||^2
  uint64_t per;            // high subsets per unit
  double* part;            // [units][g + 1], inter: [units][subsets_inter_cols(g)]
  int32_t* info;           // bit 1: a pivot failed
  // Replicates (the bootstrap, k_boot.hip): with inv_yy_rep set a launch runs `reps` replicates as its second grid
  // dimension; replicate r has its problem at the dense replicate stride behind the launch's: G + r p ldg, g + r p,
  // H + r p ldh, h + r p, inv_yy_rep[r] (device; inv_yy is not read), info[r], part + r units cols.  w and tab are
  // shared.  NULL (every other launch): one problem, nothing moves.
  const double* inv_yy_rep;
};
// reps: with GroupArgs::inv_yy_rep only (phi-only or inter, units * reps <= 2^20)
hipError_t launch_groups_enum(const GroupArgs& a, uint64_t units, uint64_t s0, uint64_t s1, bool inter,
                              hipStream_t st, int reps = 1);
// The Owen value of one group's columns (k_groups.hip's header): launch_groups_enum's phi-only launch of one problem on
// the layout of the target's refined game -- the other groups whole, the target's b columns as singletons -- with the
// weights by two counts.  tab carries the inner players' masks in GROUPS_TAB_OWEN_LO / _HI; rows 2 .. 4 of w are
// wo(r) = r! (g - 1 - r)! / g!, wi(t - 1) and wi(t) = t! (b - 1 - t)! / b! (0 outside 0 .. b - 1), each
// [GROUPS_MAX_G + 1]; rows 0 and 1 are not read.  Refuses replicates (GroupArgs::inv_yy_rep).  Of a row of the table
// the inner players' columns and b mean something: Ow_i = column i - column ng.
hipError_t launch_groups_owen(const GroupArgs& a, uint64_t units, uint64_t s0, uint64_t s1, hipStream_t st);
// Best group subset of every size (lsspa_groups_best): the units, steps and launches of launch_groups_enum, but a.part [units][g + 1] holds each unit's largest u(S) per size |S| (the number of groups) and bm
// [units][g + 1][2] its mask and a found flag, both zeroed before the first launch; every launch merges into them, and
// launch_subsets_best_reduce (p = g) takes the best over the units.  Masks in the table are in the CALLER's numbering
// (bit k = label k): gid is GroupLayout::gid, which the kernel receives by value.  Larger value wins, on equal values
// the smaller caller mask; a subset with a failed pivot of its own is no candidate.  Inside a unit the size class of a
// step is popc(s), s < per: the kernel holds GROUPS_BEST_CLASSES of them, and a per beyond 2^(GROUPS_BEST_CLASSES - 1)
// is refused (hipErrorInvalidValue), as is gh = 32 (no layout of <= 64 columns has it).
// reps: on launch_groups_enum's terms (with GroupArgs::inv_yy_rep only, 1 <= reps <= 65535, units * reps <= 2^20;
// lsspa_boot_groups_best_run): the replicates behind the launch's problem as its second grid dimension, the tables
// [reps][units][g + 1] and [reps][units][g + 1][2]; the layout, the weights and gid are the launch's.  A replicate's
// result does not depend on the launches' cut or on the replicates beside it.
constexpr int GROUPS_BEST_CLASSES = 19;   // per <= 2^18: gh <= 31 high groups over 8192 units (lsspa_api.hip asserts it)
hipError_t launch_groups_best(const GroupArgs& a, const int* gid, uint64_t units, uint64_t s0, uint64_t s1,
                              uint32_t* bm, hipStream_t st, int reps = 1);
// The T best group subsets of every size (lsspa_groups_top), 1 <= T <= GROUPS_TOP_MAX: launch_groups_best's units,
// steps, launches, candidates, order and refusals (one problem: GroupArgs::inv_yy_rep is refused), but a unit keeps per
// size a list of its T best so far, best first: a.part [units][g + 1][T] the values, tm [units][g + 1][T] the masks in
// the CALLER's numbering, tc [units][g + 1] how many entries of a list are valid.  tc is zeroed before the first launch
// (the entries need not be); every launch merges into the lists.  The order is strict (masks are unique), so the lists
// do not depend on the launches' cut.  launch_subsets_top_reduce (p = g) merges the units' lists.
constexpr int GROUPS_TOP_MAX = SUBSETS_TOP_MAX;
hipError_t launch_groups_top(const GroupArgs& a, const int* gid, uint64_t units, uint64_t s0, uint64_t s1, int T,
                             uint32_t* tm, int32_t* tc, hipStream_t st);
// K-fold cross-validation over groups (lsspa_cv_groups_*).  The `folds` fold problems of k_cv.hip lie behind a's at the
// dense replicate stride with their denominators in GroupArgs::inv_yy_rep [folds] and one info word each (the caller
// vouches for them); the attribution runs them as replicates of launch_groups_enum.
// launch_groups_cv_best: launch_groups_best's units, steps, launches, tables, candidates, order and refusals (one table:
// no second grid dimension), for u_cv(S) = u_0(S) + ... + u_{folds-1}(S), the fp64 sum in this order of the values
// launch_groups_debug gives for the fold problems; a candidate's own pivots passed in every fold, and a failed pivot
// raises a.info[fold].  launch_subsets_best_reduce (p = g) takes the best over the units.  2 <= folds <= CV_MAX_FOLDS.
hipError_t launch_groups_cv_best(const GroupArgs& a, int folds, const int* gid, uint64_t units, uint64_t s0, uint64_t s1,
                                 uint32_t* bm, hipStream_t st);
// vals[i] = u_cv(masks[i]) and, unless null, vfold[i][f] = u_f(masks[i]) by that kernel's own fold-step; masks in the
// layout's numbering
hipError_t launch_groups_cv_debug(const GroupArgs& a, int folds, const uint64_t* masks, int64_t n, double* vals,
                                  double* vfold, hipStream_t st);
size_t groups_cv_lds_bytes();      // static LDS of a workgroup of launch_groups_cv_best
size_t groups_best_lds_bytes();    // and of launch_groups_best's one-problem kernel
// launch_groups_cv_top: launch_groups_cv_best's units, steps, launches, fold-step, candidates (whose sum is also above
// -inf) and info words with launch_groups_top's lists, order and tables: a.part [units][g + 1][T], tm [units][g + 1][T]
// (CALLER masks), tc [units][g + 1], tc zeroed before the first launch; every launch merges into the lists, which do not
// depend on the cut.  launch_subsets_top_reduce (p = g) merges the units' lists.  The refusals of both siblings:
// 1 <= T <= GROUPS_TOP_MAX, 2 <= folds <= CV_MAX_FOLDS, per of at most GROUPS_BEST_CLASSES - 1 bits.
hipError_t launch_groups_cv_top(const GroupArgs& a, int folds, const int* gid, uint64_t units, uint64_t s0, uint64_t s1,
                                int T, uint32_t* tm, int32_t* tc, hipStream_t st);
size_t groups_cv_top_lds_bytes();  // static LDS of a workgroup of launch_groups_cv_top, whatever folds and T
// phi_fold[f][gid[r]] = out[f][r] - out[f][ng] of the grouped enumeration's column sums out [folds][ng + 1] (layout
// numbering; gid: GroupLayout::gid), phi[k] = their sum over f in ascending order
hipError_t launch_cv_groups_foldsum(const double* out, int ng, int folds, const int* gid, double* phi_fold, double* phi,
                                    hipStream_t st);
// The ridge path (lsspa_cv_path_shapley, lsspa_cv_path_groups_shapley): launch_cv_finalize for a block of nl ridge
// values regs [nl] (device) on the same S and nf.  Problem (l, f) is replicate l folds + f of G, g, H, h and inv_yy
// ([nl folds]...), and G of it has the bits launch_cv_finalize writes for fold f with reg = regs[l]; H, h and inv_yy of
// fold f are repeated in every l (the replicate layout has one stride).  Grid (fold, ridge value), no atomics.
constexpr int CV_PATH_MAX_REGS = 256;
hipError_t launch_cv_path_finalize(const double* S, const int32_t* nf, const double* regs, int nl, int64_t n, int p,
                                   int folds, double* G, double* g, double* H, double* h, double* inv_yy,
                                   hipStream_t st);
// launch_cv_foldsum / launch_cv_groups_foldsum for nl ridge values: out [nl][folds][cols], phi_fold [nl][folds][.],
// phi [nl][.]; row l is what the one-value launch gives on out + l folds cols
hipError_t launch_cv_path_foldsum(const double* out, int p, int folds, int nl, double* phi_fold, double* phi,
                                  hipStream_t st);
hipError_t launch_cv_path_groups_foldsum(const double* out, int ng, int folds, int nl, const int* gid, double* phi_fold,
                                         double* phi, hipStream_t st);
// Sampled attribution of the K-fold cross-validated R^2 (lsspa_cv_lift_*; k_cv.hip, launch_small_folds), p <= 127, fp64.
// Every matrix of the family has rows of CV_LIFT_LD doubles: the packed rows Xs, launch_gram's per-fold Grams S
// [folds][CV_LIFT_LD][CV_LIFT_LD], the fold problems G, H [folds][CV_LIFT_LD][CV_LIFT_LD] and g, h [folds][CV_LIFT_LD].
constexpr int CV_LIFT_MAX_P = 127, CV_LIFT_LD = 128;
// Xs[dest[i]][:] = X[i][0 .. p-1], zero up to CV_LIFT_LD, ys[dest[i]] = y[i], i < rows (dest: the rows' places when sorted
// by fold, a permutation of the rows: every place is written once)
hipError_t launch_cv_lift_pack(const void* X, int64_t ld, const void* y, int64_t rows, int p, int is_f32,
                               const int32_t* dest, double* Xs, double* ys, hipStream_t st);
// launch_cv_finalize's expressions in its order on launch_gram's buffers S; aug[f] = {2 ||y_train||^2 / (n - nf[f]) + 1,
// 2 ||y_f||^2 + 1}, the diagonals of the augmented rows
hipError_t launch_cv_lift_finalize(const double* S, const int32_t* nf, int64_t n, int p, int folds, double reg, double* G,
                                   double* g, double* H, double* h, double* inv_yy, double* aug, hipStream_t st);
// batch[s][f][k], f < folds: sample s's entry of fold f and player k from raw [n_samples * per][folds][p] -- off == NULL
// (d == p): the ordering's lift, or 0.5 * a + 0.5 * b of the pair's (per == 2); with the player map's CSR (off [d + 1],
// cols) the sum of group k's columns in ascending column order from 0.0 per ordering, then the pair combined --, and
// batch[s][folds][k] = ((e_0 + e_1) + e_2) + .. in ascending fold order.  One thread per (s, k), no atomics.
hipError_t launch_cv_lift_fold(const double* raw, int p, int folds, int per, const int32_t* off, const int32_t* cols,
                               int d, int64_t n_samples, double* batch, hipStream_t st);
// vals[i] = u(masks[i]) by the enumeration's own device code (test hook); masks in the layout's numbering
hipError_t launch_groups_debug(const GroupArgs& a, const uint64_t* masks, int64_t n, double* vals, hipStream_t st);

// Exact attribution of many responses at once (k_multi.hip), p <= MULTI_MAX_P, fp64: launch_subsets_enum's units, steps
// and weights with MULTI_RB responses carried by a wave per pass.  The `count` responses behind g, h, inv_yy are cut
// into chunks of MULTI_RB, the launch's second grid dimension; the partial table is part [chunks][MULTI_RB][units][p + 1]
// (rows of slots beyond count are never written), which launch_subsets_reduce sums with reps = chunks * MULTI_RB.
constexpr int MULTI_MAX_P = SUBSETS_MAX_P, MULTI_RB = 8;
struct MultiArgs {
  const double* G;         // [p][ldg] training Gram, shared by the responses
  const double* H;         // [p][ldh] test Gram
  int64_t ldg, ldh;
  const double* g;         // [count][p] per response
  const double* h;         // [count][p]
  const double* inv_yy;    // [count] 1 / ||y_r||^2
  const double* w;         // SubsetArgs::w (its first two rows are read)
  int p, q, count;
  double piv_tol;          // relative pivot test: a pivot d <= piv_tol G_jj raises LSSPA_INFO_NOT_PD
  uint64_t per;            // high subsets per unit
  double* part;
  int32_t* info;           // one word: G is shared
};
hipError_t launch_multi_enum(const MultiArgs& a, uint64_t units, uint64_t s0, uint64_t s1, hipStream_t st);
// vals [n][m], column r0 + r = v_r(masks[i]) of the launch's response r by the enumeration's own device code (test hook)
hipError_t launch_multi_debug(const MultiArgs& a, const uint64_t* masks, int64_t n, double* vals, int m, int r0,
                              hipStream_t st);

// ... over groups of columns (k_multi_groups.hip), g <= GROUPS_MAX_G, p <= GROUPS_MAX_P, fp64: launch_groups_enum's
// layout, units, steps and weights with MULTI_RB responses carried by a workgroup per pass.  Chunks and the partial table
// part [chunks][MULTI_RB][units][g + 1] (layout numbering, then b) as launch_multi_enum's; launch_subsets_reduce sums it
// with reps = chunks * MULTI_RB.
struct MultiGroupArgs {
  const double* G;         // [p][ldg] training Gram, shared by the responses
  const double* H;         // [p][ldh] test Gram (symmetric)
  int64_t ldg, ldh;
  const double* g;         // [count][p] per response
  const double* h;         // [count][p]
  const double* inv_yy;    // [count] 1 / ||y_r||^2
  const double* w;         // GroupArgs::w (its first two rows are read)
  const int32_t* tab;      // GroupLayout::tab on the device
  int p, ng, nb, gl, gh, ql, count;
  double piv_tol;          // relative pivot test: a pivot d <= piv_tol G_jj raises LSSPA_INFO_NOT_PD
  uint64_t per;            // high subsets per unit
  double* part;
  int32_t* info;           // one word: G is shared
};
hipError_t launch_multi_groups_enum(const MultiGroupArgs& a, uint64_t units, uint64_t s0, uint64_t s1, hipStream_t st);
// vals [n][m], column r0 + r = u_r(masks[i]) of the launch's response r by the enumeration's own device code (test hook);
// masks in the layout's numbering
hipError_t launch_multi_groups_debug(const MultiGroupArgs& a, const uint64_t* masks, int64_t n, double* vals, int m,
                                     int r0, hipStream_t st);

// Sampled attribution of many responses on one design matrix (k_small_multi.hip), p <= MLIFT_MAX_P, fp64: k_small.hip's
// LDS-resident kernel with MLIFT_RB augmented rows.  One workgroup per (ordering, chunk of MLIFT_RB responses): the grid
// is (n_samples * per_sample) x ceil(count / MLIFT_RB).  With per_sample == 2 ordering 2 s + 1 is sample s's read
// backwards and each adds half its lift vectors to sample s (lifts must be zero beforehand); with 1 they are stored.
// ng != 0 (groups of columns as the players, the kernel's GROUPED instantiation): perms are explicit, [n_samples *
// per_sample][p], rows s per_sample .. belong to sample s (never read backwards: a baseline stays in front), and a
// response's p lifts are folded in the workgroup over the player map's CSR -- group k sums cols[off[k] .. off[k+1]) in
// ascending order from 0.0, as fold_players_kernel does -- into lifts [n_samples][m][g].
constexpr int MLIFT_MAX_P = 104, MLIFT_RB = 8;
struct MultiLiftArgs {
  const double* G;         // [p][ld] training Gram, shared by the responses
  const double* H;         // [p][ld] test Gram
  int64_t ld;
  const double* g;         // [count][p] per response
  const double* h;         // [count][p]
  const double* yy;        // [count] ||y_r||^2
  double aug[2];           // diagonal of the augmented rows (train, test): above the sum of any MLIFT_RB responses'
                           // ||L^-1 g_r||^2 (||L_t^-1 h_r||^2), so that their unused trailing corner stays positive definite
  const int32_t* perms;    // [n_samples][p]; ng != 0: [n_samples * per_sample][p]
  int p, nb, n_samples, per_sample, count;   // nb = ceil((p + MLIFT_RB) / 16)
  int m;                   // responses of a sample's block of lifts (>= count)
  double* lifts;           // [n_samples][m][p]; ng != 0: [n_samples][m][ng]
  int ng, n_cols;          // groups (0: the players are the columns) and the columns they own (p less the baseline's)
  const int32_t* off;      // [ng + 1] device: the player map's CSR
  const int32_t* cols;     // [n_cols]
  double piv_tol;          // relative pivot test of the pivots j < p: d <= piv_tol G_jj raises LSSPA_INFO_NOT_PD
  int32_t* info;           // one word: G and H are shared
};
size_t multi_lift_lds_bytes(int nb, bool grouped = false);
hipError_t launch_multi_lift(const MultiLiftArgs& a, hipStream_t st);
// (n, mean, M2) [entries] += the n_b lift vectors lifts [n_b][entries]: Welford over the batch in sample order, then one
// Chan merge into the state of n_old samples.  No atomics: two runs agree bitwise.
hipError_t launch_multi_lift_stats(const double* lifts, int64_t entries, int n_b, int64_t n_old, double* mean, double* M2,
                                   hipStream_t st);

// Bootstrap of the exact attribution (k_boot.hip, boot_plan.cpp), p <= SUBSETS_MAX_P -- over groups of columns
// p <= GROUPS_MAX_P (cb = 4, 5) --, fp64.  Z = [X | y] of one side
// lives on the device as [n][ldz], ldz = 16 cb, cb = ceil((p + 1) / 16), columns beyond p zero.  A BLOCK of replicates
// is reduced at a time: counts or weights [block][n], one weighted Gram pass per side into per-slice partial sums, a
// fixed-order sum over the slices, finalise, and one enumeration grid for all its replicates.
// BootPlan, boot_plan and the bounds they work with: boot_plan.h (host code that compiles without the HIP headers).

// cnt[r][i] (uint32, zeroed by the launch) = how often row i is drawn among the n draws of replicate r0 + r, side s
hipError_t launch_boot_counts(uint64_t seed, uint64_t r0, int side, int64_t n, int reps, uint32_t* cnt, hipStream_t st);
// part[slice][r][pair][256] = sum over the slice's rows of w[r][i] z_i z_i^T, 16 x 16 blocks (bi <= bj) in the matrix
// instruction's accumulator layout; w = cnt (uint32) or wt (fp64), exactly one of them non-null, [reps][n]
hipError_t launch_boot_gram(const BootPlan& P, int side, const double* Z, int64_t n, const uint32_t* cnt,
                            const double* wt, int reps, double* part, hipStream_t st);
// wsum[r] = sum_i w[r][i] in a fixed order
hipError_t launch_boot_wsum(const uint32_t* cnt, const double* wt, int64_t n, int reps, double* wsum, hipStream_t st);
// S[r][c][c] (c = p + 1, exactly symmetric) = sum over the slices, in order, of the partials
hipError_t launch_boot_reduce(const BootPlan& P, int side, const double* part, int p, int reps, double* S,
                              hipStream_t st);
// G[r] = S_tr[:p,:p] / W + reg I (stride p), g[r] = S_tr[:p,p] / W, H[r] = S_te[:p,:p], h[r] = S_te[:p,p],
// inv_yy[r] = 1 / S_te[p][p], W = wsum_tr[r]
hipError_t launch_boot_finalize(const double* S_tr, const double* S_te, const double* wsum_tr, int p, double reg,
                                int reps, double* G, double* g, double* H, double* h, double* inv_yy, hipStream_t st);
// Z[i][0 .. p-1] = X[i][:], Z[i][p] = y[i], zero up to ldz, for rows row0 .. row0 + rows - 1 of Z; X [rows][ld], y [rows]
hipError_t launch_boot_pack(const void* X, int64_t ld, const void* y, int64_t rows, int p, int is_f32, double* Z,
                            int ldz, int64_t row0, hipStream_t st);

// The bootstrap of the sampled attribution (lsspa_boot_lift_*; BootLiftPlan: boot_plan.h), p <= BOOT_LIFT_MAX_P = 127,
// fp64: the launchers above for c = p + 1 up to 128 columns (cb up to 8), the finalise into the ordering kernels' layout
// and the per-replicate statistics.
// launch_boot_gram's part[slice][r][pair][256]: gram_form 0 goes through launch_boot_gram (cb <= 5, the existing
// instantiations); gram_form 1 (cb = 6 .. 8) is the wide form, grid (slices, reps): the four waves of a workgroup share
// rows and replicate and take the block pairs e with (e & 3) == wave.  reps <= 65535.
hipError_t launch_boot_lift_gram(const BootLiftPlan& L, int side, const double* Z, int64_t n, const uint32_t* cnt,
                                 const double* wt, int reps, double* part, hipStream_t st);
// launch_boot_reduce and launch_boot_pack for p <= BOOT_LIFT_MAX_P: the same kernels
hipError_t launch_boot_lift_reduce(const BootLiftPlan& L, int side, const double* part, int p, int reps, double* S,
                                   hipStream_t st);
hipError_t launch_boot_lift_pack(const void* X, int64_t ld, const void* y, int64_t rows, int p, int is_f32, double* Z,
                                 int ldz, int64_t row0, hipStream_t st);
// launch_boot_finalize's expressions into G, H [reps][BOOT_LIFT_LD][BOOT_LIFT_LD], g, h [reps][BOOT_LIFT_LD],
// inv_yy [reps] and aug [reps][2] = {2 S_tr[p][p] / W + 1, 2 S_te[p][p] + 1}, the augmented rows' diagonals
// (launch_cv_lift_finalize's rule).  Only rows and columns < p are written: the caller zeroes the buffers once.
hipError_t launch_boot_lift_finalize(const double* S_tr, const double* S_te, const double* wsum_tr, int p, double reg,
                                     int reps, double* G, double* g, double* H, double* h, double* inv_yy, double* aug,
                                     hipStream_t st);
// (mean, M2) [reps][d] += the n_s samples of raw [n_s * per][reps][p] (launch_small_problems' output): a sample's entry
// by launch_cv_lift_fold's rules (off == NULL, d == p: the lift, or 0.5 * a + 0.5 * b of the pair; with the player
// map's CSR the ascending-column sum from 0.0 per ordering, then the pair combined), Welford in sample order, one Chan
// merge into the state of n_old samples (launch_multi_lift_stats' expressions).  One thread per (replicate, player),
// plain stores.  samples (may be NULL): the entries [reps][n_s][d].
hipError_t launch_boot_lift_stats(const double* raw, int p, int reps, int per, const int32_t* off, const int32_t* cols,
                                  int d, int n_s, int64_t n_old, double* mean, double* M2, double* samples,
                                  hipStream_t st);

// Permutation test of the exact attribution (k_perm.hip, host_perms.cpp; PermPlan and perm_plan: boot_plan.h), p <=
// GROUPS_MAX_P, fp64.  X of one side lives on the device as Xd [n][ldx], ldx = 16 cb, cb = ceil(p / 16), columns beyond p
// zero, y as yd [n].  A block of replicates: index rows idx [reps][ldi] (uint32, entries < n), one gathered pass per
// permuted side into per-slice partial sums, a fixed-order sum over the slices into the enumeration's response slots.
// host_perms.cpp: out[i] = pi(i) of (seed, replicate r, side, n) -- Fisher-Yates on Philox4x32-10, its header has the rule
void perm_indices(uint64_t seed, uint64_t r, int side, int64_t n, uint32_t* out);
// out [reps][ldi] = the index rows of replicates r0 .. r0 + reps - 1 (entries n .. ldi - 1 zero) on up to `threads`
// native threads (at most 16)
void perm_draw_block(uint64_t seed, uint64_t r0, int reps, int side, int64_t n, int64_t ldi, uint32_t* out, int threads);
// part[slice][set][b][256] = sum over the slice's rows of X[i][16 b + ..] y[idx[16 set + ..][i]], 16 features x 16
// replicates in the matrix instruction's accumulator layout
hipError_t launch_perm_xty(const PermPlan& P, int side, const double* X, const double* y, const uint32_t* idx, int64_t n,
                           int reps, double* part, hipStream_t st);
// out[r][j] (j < p, stride p) = scale * the sum over the slices, in order, of the partials
hipError_t launch_perm_reduce(const PermPlan& P, int side, const double* part, int p, int reps, double scale, double* out,
                              hipStream_t st);
// Xd[row0 + i][:] = X[i][0 .. p-1], zero up to ldx, yd[row0 + i] = y[i]; X [rows][ld], y [rows]
hipError_t launch_perm_pack(const void* X, int64_t ld, const void* y, int64_t rows, int p, int is_f32, double* Xd, int ldx,
                            double* yd, int64_t row0, hipStream_t st);
// out[r][:] = src [p] for r < reps
hipError_t launch_perm_fill(const double* src, int p, int reps, double* out, hipStream_t st);

}  // namespace lsspa
