/* lsspa.h -- C ABI of the MI355X-native LS-SPA engine (liblsspa_hip.so).
 *
 * The reference (cvxgrp/ls-spa @ v2) has no FFI layer: its boundary is the Python
 * package surface of ls_spa/ls_spa.py.  Each entry point below names the reference
 * function(s) it stands in for; the Python host package ls-spa_amd/ls_spa binds them
 * with ctypes and re-creates the reference's own signatures on top.
 *
 * Conventions: extern "C"; plain pointers and sizes only; int status return
 * (0 = LSSPA_OK); no C++ exception crosses the boundary; the caller owns every host
 * buffer, the library owns every device buffer behind the opaque context; one context
 * per GPU; a context is not thread-safe.  All matrices are row-major.  After a
 * non-zero status lsspa_last_error() returns a description.
 */
#ifndef LSSPA_H
#define LSSPA_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSSPA_ABI_VERSION 1

#define LSSPA_OK 0
#define LSSPA_ERR_ARG 1     /* bad argument / shape */
#define LSSPA_ERR_HIP 2     /* a HIP runtime call failed */
#define LSSPA_ERR_STATE 3   /* call sequence error (no problem loaded, ...) */
#define LSSPA_ERR_NOMEM 4   /* device or host allocation failed */

#define LSSPA_F64 0
#define LSSPA_F32 1
#define LSSPA_HOST 0
#define LSSPA_DEVICE 1

/* info bit flags (lsspa_get_info) */
#define LSSPA_INFO_NOT_PD 1 /* a non-positive pivot was met in a Cholesky step */
#define LSSPA_INFO_SCAN_WAIT 4 /* an X tile gave up waiting for row p of its panel (fused lift scan): results invalid */
#define LSSPA_INFO_SUM 8 /* a sample's lifts did not sum to the R^2 of the full model (to 1e-9, more on ill-conditioned data; fp32 work: 1e-4): results invalid */

typedef struct lsspa_ctx lsspa_ctx;

int lsspa_abi_version(void);
/* NULL context: error of the last failed lsspa_create on this thread */
const char* lsspa_last_error(const lsspa_ctx* ctx);

int lsspa_create(int32_t device, lsspa_ctx** out);
int lsspa_destroy(lsspa_ctx* ctx);
/* run on a caller-provided hipStream_t (e.g. torch's current stream); NULL = library-owned */
int lsspa_set_stream(lsspa_ctx* ctx, void* hip_stream);
int lsspa_synchronize(lsspa_ctx* ctx);

/* a1 -- replaces reduce_data (ls_spa/ls_spa.py:290-318) and the |y_test|^2 of :180.
 * Forms G = X_tr^T X_tr / N + reg I, g = X_tr^T y_tr / N and, when M >= p, H = X_te^T X_te,
 * h = X_te^T y_te by one MFMA Gram pass each; when M < p the test rows themselves are
 * kept (transposed) as the test factor.  X pointers: row-major [rows][ld]; dtype applies to
 * X and y alike; location says whether the four pointers are host or device memory.
 * p <= 32767 (32-bit element counts of one p x p work matrix); a larger p is refused here with LSSPA_ERR_ARG and a
 * message naming it (the reference has no limit, ls_spa/ls_spa.py:163).  Up to p = 13567 the gather stages a whole
 * source row and the ordering in the 160 KB of LDS of a CU; beyond that a segmented (slower) gather takes over, so that
 * memory, not LDS, bounds the feature count.
 * Host arrays are never written and stay the caller's: they are read during the call only, through ordinary copies
 * (nothing of the caller's is ever page-locked: measured, the runtime's own pageable path is faster than registering
 * the arrays first).
 * No C++ exception leaves any entry point of this header: host allocation failure is LSSPA_ERR_NOMEM. */
int lsspa_reduce(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* y_train, int64_t N,
                 const void* X_test, int64_t ld_test, const void* y_test, int64_t M, int32_t p, double reg,
                 int32_t dtype, int32_t location);

/* Host seconds the last reduction from HOST arrays spent in its parts: [1] the streamed copies and Gram kernels (to
 * the last one's completion), [3] finalize (scaling, statistics reset, sync); [0] and [2] (page-locking and
 * un-locking of the caller's arrays, rounds 2-3) are always 0 now.  bench.py's e2e_breakdown. */
int lsspa_reduce_timing(const lsspa_ctx* ctx, double* seconds4);

/* a1, rows spread over several GPUs: every rank reduces the rows it holds,
 *   lsspa_reduce_partial : unscaled Gram sums of n_local training rows and m_local test rows.  M_total is the
 *                          test-row count over all ranks; if M_total < p the test rows ARE the test factor and
 *                          every rank has to pass all of them (m_local == M_total).  n_local / m_local may be 0.
 *   lsspa_reduce_buffer  : device pointer / element count (fp64) of the sums -- the all-reduce(SUM) target:
 *                          [2][P1pad][P1pad] (train, test), P1pad = p + 1 rounded up to 128; rows and columns beyond
 *                          p are zero whatever the data hold (a NaN or Inf stays in its own row and column)
 *   lsspa_reduce_finish  : G, g, H, h from the summed buffers with the global N; the context is then in the
 *                          same state as after lsspa_reduce on the stacked rows (up to summation order). */
int lsspa_reduce_partial(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* y_train,
                         int64_t n_local, const void* X_test, int64_t ld_test, const void* y_test,
                         int64_t m_local, int64_t M_total, int32_t p, int32_t dtype, int32_t location);
int lsspa_reduce_buffer(lsspa_ctx* ctx, void** device_ptr, int64_t* count);
int lsspa_reduce_finish(lsspa_ctx* ctx, int64_t N_total, double reg);

/* Load an already reduced problem (host pointers) -- the inputs square_shapley takes
 * (ls_spa/ls_spa.py:256-258) in Gram form.  G [p][p], g [p]; aug_train >= g^T G^-1 g.
 * tri != 0: H [p][p], h [p] (test Gram);  tri == 0: Ft [p][m] (transposed test factor), ytil [m]. */
int lsspa_set_reduced(lsspa_ctx* ctx, int32_t p, const double* G, const double* g, double aug_train,
                      int32_t tri, const double* H, const double* h, int32_t m, const double* Ft,
                      const double* ytil, double y_norm_sq);

/* Exact Shapley attribution of the loaded problem by enumeration of all 2^p feature subsets (p <= 32) -- the
 * definition the reference's brute-force table uses (notebooks/shapley_toy.py:100-140):
 *   phi_j = sum over S not containing j of |S|! (p - 1 - |S|)! / p! (v(S + j) - v(S)),
 *   v(S) = (2 theta_S^T h_S - theta_S^T H_SS theta_S) / ||y_test||^2,  theta_S = G_SS^-1 g_S,  v({}) = 0,
 * the R^2 of square_shapley's prefix sets (ls_spa/ls_spa.py:275-285); in rect mode H = Ft Ft^T and h = Ft ytil.
 * The phi sum to the R^2 of lsspa_full_fit; for p <= 8 they equal the mean over all p! orderings.  fp64 whatever
 * lsspa_set_precision says.  Works after lsspa_reduce, lsspa_reduce_finish or lsspa_set_reduced; p > 32 or no problem
 * loaded is LSSPA_ERR_ARG.  info: LSSPA_INFO_NOT_PD if a subset's pivot failed the engine's relative test (16 p eps).
 * Nothing of the sampling path changes: running statistics, history, flags, lanes, per-batch workspace and the info
 * word of lsspa_get_info stay as they were.  The work is split into launches of bounded length; the result is
 * bitwise reproducible (partial sums are added in a fixed order).
 *   lsspa_subsets_timing      : device milliseconds of the last call's enumeration launches (the sum of the launches'
 *                               own intervals: the gaps between them do not count), its longest launch and the
 *                               number of launches (any pointer may be NULL)
 *   lsspa_debug_subset_values : test hook -- v[i] = v(masks[i]) (bit j = feature j; masks < 2^p) by the enumeration's
 *                               own device code; a failed pivot is LSSPA_ERR_STATE */
int lsspa_subsets_shapley(lsspa_ctx* ctx, double* phi, int32_t* info);
int lsspa_subsets_timing(const lsspa_ctx* ctx, double* kernel_ms, double* max_launch_ms, int64_t* launches);
int lsspa_debug_subset_values(lsspa_ctx* ctx, const uint64_t* masks, int64_t n, double* v);

/* Exact pairwise Shapley interaction index of the loaded problem, from the same enumeration of all 2^p subsets
 * (p <= 32) and the same v:
 *   I_ij = sum over S without i and j of |S|! (p - 2 - |S|)! / (p - 1)! (v(S + i + j) - v(S + i) - v(S + j) + v(S)).
 * inter [p][p] is symmetric, holds the raw index I_ij off the diagonal and 0 on it (SHAP's matrix has I_ij / 2 off the
 * diagonal and phi_i minus the rest of row i on it; the Python driver forms it).  phi [p] is bitwise the phi of
 * lsspa_subsets_shapley.  Errors, the p <= 32 limit, info, fp64, bounded launches, bitwise reproducibility and "nothing
 * of the sampling path changes" are those of lsspa_subsets_shapley; the two calls share their buffers, and this call
 * leaves its timing where lsspa_subsets_timing reads it.  The partial table is p (p + 3) / 2 + 2 columns wide: about
 * 37 MB of device memory at p = 32. */
int lsspa_subsets_interactions(lsspa_ctx* ctx, double* phi /* [p] */, double* inter /* [p*p] */, int32_t* info);

/* Best subset of every size by the same v, over the same enumeration of all 2^p subsets (p <= 32): for k = 0 .. p
 *   v[k] = max over the candidates K with |K| = k of v(K),   masks[k] = the K that attains it (bit j = feature j),
 * an arg-max, not a sum: what lsspa_subsets_shapley folds away.  v[k] has the very bits lsspa_debug_subset_values
 * returns for masks[k].
 * Ties: the larger value wins, on equal values the numerically smaller mask -- a total order, so the result does not
 * depend on how the work is cut into units and launches.
 * Candidates: the subsets K with (K & include) == include (columns every model must contain; bits at or above p are
 * LSSPA_ERR_ARG) whose own pivots all passed the relative test.  A subset with a failed pivot is not a candidate and
 * raises LSSPA_INFO_NOT_PD in info (whether or not it contains include); a NaN value never wins.  found[k] = 0: no
 * subset of size k was a candidate (k < popcount(include), or every one failed a pivot); v[k] is then NaN and masks[k]
 * 0.  With include == 0, v[0] = 0.0 with the empty mask.
 * Limits and errors are those of lsspa_subsets_shapley (p > 32, no problem loaded: LSSPA_ERR_ARG); NULL v, masks or
 * found is LSSPA_ERR_ARG, info may be NULL.  fp64, bounded launches as that call cuts them, no atomics on the table:
 * two calls agree bitwise.  It shares lsspa_subsets_shapley's buffers (a call of that before and after this one
 * agrees bitwise) and leaves its timing where lsspa_subsets_timing reads it; nothing of the sampling path changes. */
int lsspa_subsets_best(lsspa_ctx* ctx, uint32_t include, double* v /* [p+1] */, uint32_t* masks /* [p+1] */,
                       uint8_t* found /* [p+1] */, int32_t* info);

/* The T best subsets of every size (1 <= T <= 16): lsspa_subsets_best's enumeration, v, candidates (include, own pivots
 * passed, NaN never listed) and order, keeping per size k = 0 .. p not one winner but a list,
 *   v[k][r], masks[k][r], r < count[k] = min(T, number of candidates of size k),
 * best first: the larger value, on equal values the numerically smaller mask.  Masks are unique, so the order is strict
 * and the list does not depend on how the work is cut into units and launches.  Entries past count[k] are NaN / 0.
 * Rank 0 is bitwise lsspa_subsets_best's (value, mask, found) for the same include; every listed value has the very
 * bits lsspa_debug_subset_values returns for its mask; the lists of a call with T are the first T ranks of a call with
 * a larger T; two calls agree bitwise (no atomics on the table).
 * Limits, refusals and messages are lsspa_subsets_best's (p > 32, no problem loaded, include bits at or above p:
 * LSSPA_ERR_ARG); T outside 1 .. 16 is LSSPA_ERR_ARG naming the limit; NULL v, masks or count is LSSPA_ERR_ARG, info may
 * be NULL (LSSPA_INFO_NOT_PD as there).  It shares lsspa_subsets_shapley's buffers (a call of that, or of
 * lsspa_subsets_best, before and after this one agrees bitwise) and leaves its timing where lsspa_subsets_timing reads
 * it; nothing of the sampling path, the grouped state or the bootstrap store changes.
 * Device memory: the units' lists, units (p + 1) of them with units = min(2^(p - 6), 8192), 12 bytes an entry (value,
 * mask) and 4 a list (count): 8192 x 33 x (12 x 16 + 4) bytes = 53 MB at p = 32 and T = 16.
 *   lsspa_debug_subsets_top_plan : host only, no context, no GPU -- units, high subsets per unit, steps of a unit per
 *                     launch, launches, sizes one unit can hold, bytes of the table, rounds of the final reduction (T),
 *                     0; from the functions the call itself uses.  p outside 1 .. 32 or T outside 1 .. 16 is
 *                     LSSPA_ERR_ARG. */
int lsspa_subsets_top(lsspa_ctx* ctx, uint32_t include, int32_t T, double* v /* [p+1][T] */,
                      uint32_t* masks /* [p+1][T] */, int32_t* count /* [p+1] */, int32_t* info);
int lsspa_debug_subsets_top_plan(int32_t p, int32_t T, int64_t* plan /* [8] */);

/* Exact Shapley attribution over GROUPS of columns: the players are the g <= 32 groups, the problem has p <= 64 columns.
 * labels[j] in {-1, 0 .. g-1} for every column j: group k is {j : labels[j] == k} (none may be empty), the columns
 * labelled -1 are the baseline B, part of every model and given no attribution.  With F(S) = B + the columns of the
 * groups in S and u(S) = v(F(S)), v as above,
 *   phi_k = sum over S not containing k of |S|! (g - 1 - |S|)! / g! (u(S + k) - u(S)),   k = 0 .. g-1.
 * The phi sum to R^2(all columns) - R^2(B alone).  All-singleton labels 0 .. p-1 give lsspa_subsets_shapley's phi.
 * The cost is set by g (2^g group subsets), not by p.  Everything else as lsspa_subsets_shapley: fp64, any reduction,
 * bounded launches, bitwise reproducible, LSSPA_INFO_NOT_PD in info, nothing of the sampling path and nothing of
 * lsspa_subsets_shapley's state touched.  g > 32, p > 64, a label outside -1 .. g-1, an empty group, g < 1 or no
 * problem loaded is LSSPA_ERR_ARG (lsspa_last_error names it).
 *   lsspa_groups_timing      : as lsspa_subsets_timing, for the last lsspa_groups_shapley or
 *                              lsspa_groups_interactions call (and lsspa_groups_owen, _best, _top)
 *   lsspa_debug_group_values : test hook -- u[i] = u(masks[i]) (bit k = group k; masks < 2^g) by the enumeration's own
 *                              device code; a failed pivot is LSSPA_ERR_STATE */
int lsspa_groups_shapley(lsspa_ctx* ctx, const int32_t* labels, int32_t g, double* phi /* [g] */, int32_t* info);
int lsspa_groups_timing(const lsspa_ctx* ctx, double* kernel_ms, double* max_launch_ms, int64_t* launches);
int lsspa_debug_group_values(lsspa_ctx* ctx, const int32_t* labels, int32_t g, const uint64_t* masks, int64_t n,
                             double* u);

/* Exact pairwise Shapley interaction index between GROUPS of columns, from the same enumeration of all 2^g group
 * subsets (g <= 32, p <= 64) and the same u as lsspa_groups_shapley:
 *   I_kl = sum over S without k and l of |S|! (g - 2 - |S|)! / (g - 1)! (u(S + k + l) - u(S + k) - u(S + l) + u(S)).
 * inter [g][g], indexed by the caller's labels like phi, is symmetric, holds the raw index I_kl off the diagonal and 0
 * on it (SHAP's matrix as for lsspa_subsets_interactions; its rows sum to phi and the whole to R^2(all columns) -
 * R^2(B alone)).  phi [g] is bitwise the phi of lsspa_groups_shapley.  All-singleton labels 0 .. p-1 give
 * lsspa_subsets_interactions' index.  Errors, limits, labels, info, fp64, bounded launches, bitwise reproducibility and
 * "nothing of the sampling path and nothing of lsspa_subsets_shapley's state touched" are those of lsspa_groups_shapley
 * (NULL inter is LSSPA_ERR_ARG); the two calls share their buffers, and this call leaves its timing where
 * lsspa_groups_timing reads it.  The partial table is g (g + 3) / 2 + 2 columns wide: 8192 x 562 doubles, about 37 MB
 * of device memory, at g = 32. */
int lsspa_groups_interactions(lsspa_ctx* ctx, const int32_t* labels, int32_t g, double* phi /* [g] */,
                              double* inter /* [g*g] */, int32_t* info);

/* Best group subset of every size: lsspa_subsets_best with the groups of lsspa_groups_shapley as the players, over the
 * same enumeration of all 2^g group subsets (g <= 32, p <= 64) and the same u.  For k = 0 .. g
 *   u[k] = max over the candidates S with |S| = k groups of u(S),   masks[k] = the S that attains it (bit k = group k,
 *   the caller's labels),
 * so that size 0 is the baseline alone: u[0] = R^2(B), or 0.0 without a baseline.  u[k] has the very bits
 * lsspa_debug_group_values returns for masks[k].
 * Ties: the larger value wins, on equal values the numerically smaller mask in the caller's numbering -- a total order,
 * so the result depends neither on how the work is cut into units and launches nor on which groups the layout makes
 * low.  Candidates: the group subsets whose own pivots all passed the relative test; one with a failed pivot is no
 * candidate and raises LSSPA_INFO_NOT_PD in info, and a NaN value never wins.  found[k] = 0: no subset of k groups was
 * a candidate; u[k] is then NaN and masks[k] 0.
 * Labels, limits, refusals and their messages are lsspa_groups_shapley's; NULL u, masks or found is LSSPA_ERR_ARG, info
 * may be NULL.  fp64, bounded launches as that call cuts them, no atomics on the table: two calls agree bitwise.  It
 * shares lsspa_groups_shapley's buffers (a call of that before and after this one agrees bitwise) and leaves its timing
 * where lsspa_groups_timing reads it; nothing of the sampling path or of lsspa_subsets_shapley's state changes.
 *   lsspa_debug_groups_best_plan : host only (no context, no GPU) -- plan[0 .. 7] = gl, gh, ql (low groups, high groups,
 *                                  low columns of the labels' layout), nb (baseline columns), units, per (high subsets a
 *                                  unit; units x per = 2^gh), launches and the size classes a unit holds
 *                                  (log2(per) + 1).  Labels that lsspa_groups_best would refuse: LSSPA_ERR_ARG. */
int lsspa_groups_best(lsspa_ctx* ctx, const int32_t* labels, int32_t g, double* u /* [g+1] */,
                      uint32_t* masks /* [g+1] */, uint8_t* found /* [g+1] */, int32_t* info);
int lsspa_debug_groups_best_plan(const int32_t* labels, int32_t p, int32_t g, int64_t* plan /* [8] */);

/* The T best group subsets of every size (1 <= T <= 16): lsspa_groups_best's enumeration, u, candidates (own pivots
 * passed, NaN never listed) and order, keeping per size k = 0 .. g (the number of groups) not one winner but a list,
 *   u[k][r], masks[k][r], r < count[k] = min(T, number of candidates of k groups),
 * best first: the larger value, on equal values the numerically smaller mask in the caller's numbering (bit k = label
 * k).  Masks are unique, so the order is strict and the list depends neither on how the work is cut into units and
 * launches nor on which groups the layout makes low.  Entries past count[k] are NaN / 0.  Rank 0 is bitwise
 * lsspa_groups_best's (value, mask, found); every listed value has the very bits lsspa_debug_group_values returns for
 * its mask; the lists of a call with T are the first T ranks of a call with a larger T; two calls agree bitwise (no
 * atomics on the table).
 * Labels, limits, refusals and their messages are lsspa_groups_best's; T outside 1 .. 16 is LSSPA_ERR_ARG naming the
 * limit; NULL labels, u, masks or count is LSSPA_ERR_ARG, info may be NULL (LSSPA_INFO_NOT_PD as there).  It shares
 * lsspa_groups_shapley's buffers (a call of that, or of lsspa_groups_best, before and after this one agrees bitwise)
 * and leaves its timing where lsspa_groups_timing reads it; nothing of the sampling path, of lsspa_subsets_shapley's
 * state or of the bootstrap store changes.
 * Device memory: the units' lists, units (g + 1) of them with units = min(2^gh, 8192), 12 bytes an entry (value, mask)
 * and 4 a list (count): at most 8192 x 33 x (12 x 16 + 4) bytes = 53 MB.
 *   lsspa_debug_groups_top_plan : host only (no context, no GPU) -- plan[0 .. 9] = gl, gh, ql, nb, units, per (as
 *                                 lsspa_debug_groups_best_plan's), steps of a unit per launch, launches, the most sizes
 *                                 one unit holds (at most 25) and the bytes of the table; from the function the call
 *                                 itself uses.  Labels that lsspa_groups_best would refuse, or T outside 1 .. 16:
 *                                 LSSPA_ERR_ARG. */
int lsspa_groups_top(lsspa_ctx* ctx, const int32_t* labels, int32_t g, int32_t T, double* u /* [g+1][T] */,
                     uint32_t* masks /* [g+1][T] */, int32_t* count /* [g+1] */, int32_t* info);
int lsspa_debug_groups_top_plan(const int32_t* labels, int32_t p, int32_t g, int32_t T, int64_t* plan /* [10] */);

/* Exact Owen values: the attribution of every COLUMN with the groups as coalition structure, the two-level Shapley
 * value.  Labels, B, u and v as lsspa_groups_shapley's.  For a column i of group k, with B_k the group's columns,
 * b = |B_k| and cols(R) the columns of the groups in R,
 *   Ow_i = sum over R within groups \ {k}, T within B_k \ {i} of
 *          |R|! (g - 1 - |R|)! / g!  |T|! (b - 1 - |T|)! / b!  (v(B + cols(R) + T + i) - v(B + cols(R) + T)):
 * the mean of the column's lift over the orderings in which the baseline comes first and every group's columns are
 * contiguous.  The Owen values of a group's columns sum to the group's phi, all of them to R^2(all columns) -
 * R^2(B alone).  All-singleton labels give lsspa_subsets_shapley's phi, g = 1 the Shapley value of the group's columns
 * with the baseline eliminated.
 *   owen [p] : Ow_i per column, 0.0 on baseline columns; a group of one column gets its phi.
 *   phi [g]  : the group game's Shapley values, bitwise lsspa_groups_shapley's.
 * Per group of b >= 2 columns one enumeration of its refined game -- the other g - 1 groups whole and the group's
 * columns as singletons, 2^(g - 1 + b) subsets -- by lsspa_groups_shapley's kernel with the weight of a subset looked up
 * by two counts.  Hence one limit more: g - 1 + max_k b_k <= 32 players, refused with LSSPA_ERR_ARG naming the first
 * offending group.  Everything else -- labels, refusals and their messages, fp64, bounded launches, bitwise
 * reproducibility, nothing of the sampling path or of lsspa_subsets_shapley's state touched -- is lsspa_groups_shapley's,
 * whose buffers this call shares.  info: the OR over all enumerations.  lsspa_groups_timing afterwards reports the sums
 * over all launches of the call (the group game's included) and its longest launch.
 *   lsspa_debug_owen_plan : host only (no context, no GPU) -- per target group k, plan[k][0 .. 7] = players of its
 *                           refined game, gl, gh, ql of that game's layout, inner players (the group's columns) among the
 *                           low and among the high players, high subsets enumerated (units x per = 2^gh), launches (0
 *                           for a group of one column, which has no enumeration of its own).  Labels that
 *                           lsspa_groups_owen would refuse: LSSPA_ERR_ARG. */
int lsspa_groups_owen(lsspa_ctx* ctx, const int32_t* labels, int32_t g, double* owen /* [p] */, double* phi /* [g] */,
                      int32_t* info);
int lsspa_debug_owen_plan(const int32_t* labels, int32_t p, int32_t g, int64_t* plan /* [g][8] */);

/* Bootstrap of the exact attribution (p <= 32): how far would phi move had the rows been another draw from the same
 * population?  Replicate r resamples the rows of a side with replacement -- or takes the caller's weights -- and its
 * reduced problem is a WEIGHTED Gram of rows that stay on the device: with z = [x, y], S = sum_i w_i z_i z_i^T per side and
 * W = sum_i w_i of the training side,
 *   G = S_tr[:p,:p] / W + reg I,  g = S_tr[:p,p] / W,  H = S_te[:p,:p],  h = S_te[:p,p],  ||y||^2 = S_te[p][p],
 * then lsspa_subsets_shapley's enumeration, all replicates of a block in one grid.  fp64 throughout.
 *   lsspa_boot_load : keeps [X | y] of both sides on the device in fp64 (arguments as lsspa_reduce's).  p > 32 is
 *                     LSSPA_ERR_ARG naming the limit; N, M < 2^31.  The loaded problem, the running statistics and the
 *                     exact enumerations' state are not touched, now or by any call below; a reduction or
 *                     lsspa_set_reduced does not free the bootstrap data, and lsspa_boot_free does not touch the problem.
 *   lsspa_boot_run  : replicates first .. first + R - 1 of the bootstrap keyed by `seed`; phi [R][p], r2 [R] (R^2 of the
 *                     replicate's full model, by a Cholesky solve of its G on the host; NaN where that fails), info [R].
 *                     w_train host fp64 [R][N] / w_test [R][M]: weights instead of counts on that side, finite, >= 0 and
 *                     with a positive sum in every replicate, else LSSPA_ERR_ARG (Bayesian bootstrap, survey weights,
 *                     a jackknife by zero weights, weight 1 everywhere for a side that is not resampled).  NULL: the
 *                     counts below.  A replicate whose pivot fails the engine's relative test (16 p eps) has
 *                     LSSPA_INFO_NOT_PD in ITS word, and its phi is whatever came out; the others are unaffected.
 *                     block: replicates reduced and enumerated together, 0 = as many as 256 MB hold (counts or weights of
 *                     both sides, Gram partials, the enumeration's partial table; at most 1024), a larger request is cut
 *                     to that; R itself is unlimited.  Results do not depend on block or on how a run is cut into calls
 *                     (`first`), and two runs agree bitwise: integer atomics for the counts, no floating-point atomics,
 *                     row slices that depend on the rows alone, sums in a fixed order.  LSSPA_ERR_STATE before a load.
 *   Counts: draw t = 0 .. n-1 of replicate r on side s (0 train, 1 test; n = N or M) picks row
 *                     (uint64(word) * n) >> 32, word = output word t % 4 of Philox4x32-10 with key = (seed & 0xffffffff,
 *                     seed >> 32) and counter = (t / 4, s, r & 0xffffffff, r >> 32); cnt[i] = draws that picked row i.
 *                     Row i has probability within n / 2^32 (relative) of 1 / n.  tests/boot_ref.py restates it on
 *                     tests/philox_ref.py bit for bit.
 *   lsspa_boot_timing       : kernel ms of the last run: counts (or the upload of the caller's weights), Gram (both
 *                     passes, their sums, finalise) and enumeration (any pointer may be NULL)
 *   lsspa_boot_debug_counts : test hook -- the counts [n] of replicate r on `side`
 *   lsspa_boot_debug_grams  : test hook -- S_train, S_test [R][p+1][p+1] and wsum [R] (training side) before finalise;
 *                     NULL weights on a side: weight 1 on every row (any output pointer may be NULL)
 *   lsspa_debug_boot_plan   : host only (no context, no GPU) -- how a run of R replicates on N / M rows at p features is
 *                     cut: plan15 = cb (16-column blocks of [X | y]), ldz, block pairs, replicates per wave, rows per
 *                     slice train / test, slices train / test, bytes per replicate, replicates per block, blocks,
 *                     replicates per enumeration launch, units, high subsets per unit, steps per launch */
int lsspa_boot_load(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* y_train, int64_t N,
                    const void* X_test, int64_t ld_test, const void* y_test, int64_t M, int32_t p, double reg,
                    int32_t dtype, int32_t location);
int lsspa_boot_run(lsspa_ctx* ctx, int64_t R, uint64_t seed, int64_t first, const double* w_train /* [R][N] or NULL */,
                   const double* w_test /* [R][M] or NULL */, int64_t block, double* phi /* [R][p] */,
                   double* r2 /* [R] */, int32_t* info /* [R] */);
int lsspa_boot_free(lsspa_ctx* ctx);
int lsspa_boot_timing(const lsspa_ctx* ctx, double* counts_ms, double* gram_ms, double* enum_ms);
int lsspa_boot_debug_counts(lsspa_ctx* ctx, uint64_t seed, uint64_t r, int32_t side, uint32_t* out /* [n] */);
int lsspa_boot_debug_grams(lsspa_ctx* ctx, int64_t R, const double* w_train, const double* w_test,
                           double* S_train /* [R][c][c] */, double* S_test, double* wsum /* [R] */);
int lsspa_debug_boot_plan(int64_t R, int64_t N, int64_t M, int32_t p, int64_t block, int64_t* plan15);

/* The bootstrap over groups of columns (g <= 32 groups, p <= 64 columns, label -1 = an always-included baseline): the
 * replicates of lsspa_boot_run -- the same rows, counts, weights and weighted Grams -- attributed by
 * lsspa_groups_shapley's enumeration of the 2^g group subsets, all replicates of a block in one grid.
 *   lsspa_boot_groups_load : lsspa_boot_load for p <= 64 (p > 64 is LSSPA_ERR_ARG naming the limit).  The same device
 *                     store: one set of bootstrap rows per context, freed by lsspa_boot_free.  After a load with p > 32
 *                     lsspa_boot_run is LSSPA_ERR_ARG; lsspa_boot_debug_grams, lsspa_boot_debug_counts and
 *                     lsspa_boot_timing work as before.
 *   lsspa_boot_groups_run  : after either load.  labels [p] as lsspa_groups_shapley's (bad labels: LSSPA_ERR_ARG).  R,
 *                     seed, first, w_train, w_test, block: lsspa_boot_run's -- draw (seed, r, side, t) is the same
 *                     function, so a seed resamples the same rows with and without groups.  phi [R][g] in label order;
 *                     r2 [R] the R^2 of the replicate's full model and r2_base [R] that of its baseline columns alone (0
 *                     without a baseline), both by Cholesky solves on the host (NaN where one fails): the phi of a
 *                     replicate sum to r2 - r2_base.  info [R] as lsspa_boot_run's.  Results do not depend on block or on
 *                     `first`, and two runs agree bitwise: a unit's high subsets are cut into launches by the layout
 *                     alone, as lsspa_groups_shapley cuts them, never by R, block or the replicates a launch takes.  A
 *                     replicate's phi has the bits lsspa_groups_shapley returns for its reduced problem.
 *   lsspa_debug_boot_groups_plan : host only (no context, no GPU) -- lsspa_debug_boot_plan's fifteen numbers for a run
 *                     over the groups of labels [p]: cb up to 5 (p + 1 = 65 columns), one replicate a wave from cb = 4,
 *                     units / per / steps over the 2^gh high group subsets as the one-problem enumeration cuts them
 *                     (a function of the labels alone), replicates per launch within that call's work bound and
 *                     units * replicates <= 2^20.  Bad labels or sizes: LSSPA_ERR_ARG. */
int lsspa_boot_groups_load(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* y_train, int64_t N,
                           const void* X_test, int64_t ld_test, const void* y_test, int64_t M, int32_t p, double reg,
                           int32_t dtype, int32_t location);
int lsspa_boot_groups_run(lsspa_ctx* ctx, const int32_t* labels /* [p] */, int32_t g, int64_t R, uint64_t seed,
                          int64_t first, const double* w_train /* [R][N] or NULL */,
                          const double* w_test /* [R][M] or NULL */, int64_t block, double* phi /* [R][g] */,
                          double* r2 /* [R] */, double* r2_base /* [R] */, int32_t* info /* [R] */);
int lsspa_debug_boot_groups_plan(int64_t R, int64_t N, int64_t M, const int32_t* labels /* [p] */, int32_t p, int32_t g,
                                 int64_t block, int64_t* plan15);

/* Bootstrap of the exact pairwise interaction values: the replicates of lsspa_boot_run / lsspa_boot_groups_run -- the
 * same loaded rows, draws, weights, weighted Grams, finalise, r2, r2_base, info, `first`, `block` and refusals --
 * enumerated by the interaction instantiation of the same kernels, all replicates of a launch in one grid.
 *   lsspa_boot_interactions_run : after lsspa_boot_load (a load with p > 32 is LSSPA_ERR_ARG naming the limit).  phi
 *                     [R][p] is bitwise lsspa_boot_run's for the same seed; inter [R][p][p] is replicate r's raw index
 *                     I_ij = T0 - T1_i - T1_j + T2_ij as lsspa_subsets_interactions returns it (symmetric, 0 on the
 *                     diagonal), formed on the host by that call's code.  A replicate's phi and inter have the bits
 *                     lsspa_subsets_interactions returns for its reduced problem, whatever R, block and first are: a
 *                     unit's high subsets are cut into launches by p alone, as the one-problem call cuts them.
 *   lsspa_boot_groups_interactions_run : after either load; labels, g as lsspa_boot_groups_run's.  phi [R][g] and
 *                     inter [R][g][g] in label order, with the bits of lsspa_groups_interactions on the replicate's
 *                     reduced problem; phi is bitwise lsspa_boot_groups_run's.
 *   The partial table is d (d + 3) / 2 + 2 columns wide (d = p or g; 37 MB a replicate at d = 32): it is kept for the
 *   replicates of one enumeration launch only, beside the block's 256 MB, so a block is not cut to a few replicates.
 *   lsspa_boot_timing reports these runs like the others.
 *   lsspa_debug_boot_inter_plan, lsspa_debug_boot_groups_inter_plan : host only -- the fifteen numbers of
 *                     lsspa_debug_boot_plan / lsspa_debug_boot_groups_plan for these runs.  Bytes per replicate leave
 *                     the partial table out: block * bytes + replicates per launch * units * columns * 8 <= 256 MB
 *                     (or block = 1).  steps is a function of the players alone; units * replicates per launch *
 *                     steps <= 2^20. */
int lsspa_boot_interactions_run(lsspa_ctx* ctx, int64_t R, uint64_t seed, int64_t first,
                                const double* w_train /* [R][N] or NULL */, const double* w_test /* [R][M] or NULL */,
                                int64_t block, double* phi /* [R][p] */, double* inter /* [R][p][p] */,
                                double* r2 /* [R] */, int32_t* info /* [R] */);
int lsspa_boot_groups_interactions_run(lsspa_ctx* ctx, const int32_t* labels /* [p] */, int32_t g, int64_t R,
                                       uint64_t seed, int64_t first, const double* w_train /* [R][N] or NULL */,
                                       const double* w_test /* [R][M] or NULL */, int64_t block,
                                       double* phi /* [R][g] */, double* inter /* [R][g][g] */, double* r2 /* [R] */,
                                       double* r2_base /* [R] */, int32_t* info /* [R] */);
int lsspa_debug_boot_inter_plan(int64_t R, int64_t N, int64_t M, int32_t p, int64_t block, int64_t* plan15);
int lsspa_debug_boot_groups_inter_plan(int64_t R, int64_t N, int64_t M, const int32_t* labels /* [p] */, int32_t p,
                                       int32_t g, int64_t block, int64_t* plan15);

/* Bootstrap of the best-subset selection (p <= 32): how stable is the chosen model?  The replicates of lsspa_boot_run --
 * the same loaded rows, draws, weights, weighted Grams, finalise, r2, info, `first`, `block` and refusals (a seed
 * resamples the same rows) -- each searched by lsspa_subsets_best's enumeration, all replicates of a launch in one grid.
 *   lsspa_boot_best_run : after lsspa_boot_load (a load with p > 32 is LSSPA_ERR_ARG naming the limit).  include:
 *                     lsspa_subsets_best's mask, refused like there.  Of replicate r, v [r][k] is the largest
 *                     out-of-sample R^2 among its subsets of size k = 0 .. p, masks [r][k] that subset (bit j = feature
 *                     j) and found [r][k] whether the size had a candidate (else v is NaN and the mask 0): the bits
 *                     lsspa_subsets_best returns for the replicate's reduced problem, whatever R, block and first are --
 *                     the larger value wins, then the smaller mask, a total order that no cut of the work can show in.
 *                     A replicate whose pivot fails has LSSPA_INFO_NOT_PD in its own word only; the subsets whose own
 *                     pivots failed are no candidates, every other subset of that replicate still is.
 *   lsspa_boot_timing reports the run like the others.
 *   lsspa_debug_boot_best_plan : host only -- the fifteen numbers of lsspa_debug_boot_plan for this run.  An entry of the
 *                     enumeration's table takes 16 bytes (value, mask, found) against the 8 of lsspa_boot_run's, counted
 *                     in the bytes per replicate: block * bytes <= 256 MB (or block = 1); units * replicates per launch
 *                     * steps <= 2^20; high subsets per unit <= 2^13. */
int lsspa_boot_best_run(lsspa_ctx* ctx, int64_t R, uint64_t seed, int64_t first,
                        const double* w_train /* [R][N] or NULL */, const double* w_test /* [R][M] or NULL */,
                        int64_t block, uint32_t include, double* v /* [R][p + 1] */, uint32_t* masks /* [R][p + 1] */,
                        uint8_t* found /* [R][p + 1] */, double* r2 /* [R] */, int32_t* info /* [R] */);
int lsspa_debug_boot_best_plan(int64_t R, int64_t N, int64_t M, int32_t p, int64_t block, int64_t* plan15);

/* Bootstrap of the best-subset selection over groups of columns (g <= 32 groups, p <= 64 columns, label -1 = the
 * always-included baseline).  The replicates of lsspa_boot_groups_run -- the same loaded rows, draws, weights, weighted
 * Grams, finalise, r2, r2_base, info, `first`, `block` and refusals (a seed resamples the same rows) -- each searched by
 * lsspa_groups_best's enumeration of the 2^g group subsets, all replicates of a launch in one grid.
 *   lsspa_boot_groups_best_run : after either load.  labels [p], g as lsspa_groups_best's, refused with its messages.
 *                     Of replicate r, u [r][k] is the largest out-of-sample R^2 among its sets of k = 0 .. g groups
 *                     (beside the baseline), masks [r][k] that set (bit j = label j) and found [r][k] whether the size
 *                     had a candidate (else u is NaN and the mask 0): the bits lsspa_groups_best returns for the
 *                     replicate's reduced problem, whatever R, block, first and the cut into launches are -- the larger
 *                     value wins, then the smaller mask, a total order that no cut of the work can show in.  A replicate
 *                     whose pivot fails has LSSPA_INFO_NOT_PD in its own word only; the sets whose own pivots failed
 *                     are no candidates, every other set of that replicate still is.
 *   lsspa_boot_timing reports the run like the others.
 *   lsspa_debug_boot_groups_best_plan : host only -- the fifteen numbers of lsspa_debug_boot_groups_plan for this run.
 *                     An entry of the enumeration's table takes 16 bytes (value, mask, found), counted in the bytes per
 *                     replicate: block * bytes <= 256 MB (or block = 1).  steps is the one-problem call's; replicates
 *                     per launch fill what it leaves of that call's work bound, units * replicates <= 2^20; high subsets
 *                     per unit <= 2^18.  Bad labels or sizes: LSSPA_ERR_ARG. */
int lsspa_boot_groups_best_run(lsspa_ctx* ctx, const int32_t* labels /* [p] */, int32_t g, int64_t R, uint64_t seed,
                               int64_t first, const double* w_train /* [R][N] or NULL */,
                               const double* w_test /* [R][M] or NULL */, int64_t block, double* u /* [R][g + 1] */,
                               uint32_t* masks /* [R][g + 1] */, uint8_t* found /* [R][g + 1] */, double* r2 /* [R] */,
                               double* r2_base /* [R] */, int32_t* info /* [R] */);
int lsspa_debug_boot_groups_best_plan(int64_t R, int64_t N, int64_t M, const int32_t* labels /* [p] */, int32_t p,
                                      int32_t g, int64_t block, int64_t* plan15);

/* K-FOLD CROSS-VALIDATION (p <= 32, 2 <= K <= 32 folds, fp64, no groups): one data set, no split to choose.  Rows
 * z_i = [x_i, y_i], i < N; fold f holds the rows with fold_ids[i] == f (n_f >= 1 of them), S_f = sum_{i in f} z_i z_i^T.
 * Fold problem f is tested on fold f and trained on the other rows, in the bootstrap's normalisation with W_f = N - n_f:
 *   G_f = (sum_{j != f} S_j)[:p,:p] / W_f + reg I,  g_f = (sum_{j != f} S_j)[:p,p] / W_f   (j ascending: sums, not a
 *   total minus S_f),  H_f = S_f[:p,:p],  h_f = S_f[:p,p],
 * and every fold divides by the same POOLED ||y||^2 = sum_j S_j[p][p] (j ascending): with one denominator the folds'
 * values add up to the cross-validated R^2 exactly,
 *   v_cv(K) = sum_f v_f(K) (f ascending, fp64) = 1 - sum_f ||y_f - X_f theta_K^(-f)||^2 / ||y||^2,
 * v_f what lsspa_debug_subset_values gives for problem f.  The Shapley value is linear in the game:
 * phi_cv = sum_f phi_f (f ascending), and its entries sum to v_cv(all columns).
 *   lsspa_cv_load   : packs [X | y] once (arguments as lsspa_reduce's for one side; fold_ids a HOST array [N]), writes
 *                     the folds' indicator weights on the device from the labels (no [K][N] array crosses the bus),
 *                     runs the bootstrap's weighted Gram pass for S_f and finalises the K problems.  Refused before any
 *                     GPU work with LSSPA_ERR_ARG naming the limit: p > 32, K outside 2 .. 32, a label outside
 *                     0 .. K-1, an empty fold, sum y^2 = 0 (rows on the device: that one after the Gram pass).
 *                     The loaded problem, the statistics, the enumerations' and the bootstrap's state are not touched,
 *                     now or by any call below.
 *   lsspa_cv_shapley: phi [p] = phi_cv, phi_fold [K][p] (row f has the bits lsspa_subsets_shapley gives for problem f:
 *                     the same kernel, cut into launches as that call cuts it), r2_fold [K] = v_f(all columns), info
 *                     [K]: LSSPA_INFO_NOT_PD in the word of the fold a pivot failed in.
 *   lsspa_cv_best   : lsspa_subsets_best by v_cv: v [p+1], masks, found as there -- the larger v_cv wins, on equal
 *                     values the smaller mask, so the result depends on no cut --, candidates: (K & include) == include
 *                     and the subset's own pivots passed in EVERY fold (info [K] says which fold failed).  v[k] has the
 *                     bits of lsspa_debug_cv_values for masks[k].  v_fold [p+1][K]: the winner's per-fold values (NaN
 *                     where found[k] = 0).  steps = 0: the plan's steps of a unit per launch; > 0: that many (a test's
 *                     way to cut a small p into several launches).  No floating-point atomics: two calls agree bitwise.
 *   lsspa_cv_top    : lsspa_subsets_top by v_cv: per size k the T best subsets (1 <= T <= 16), best first, in
 *                     lsspa_cv_best's order and over its candidates, whose sum is also above -inf (so never NaN).  v
 *                     [p+1][T], masks [p+1][T], count [p+1] = min(T, candidates of size k); NaN / 0 past count[k].
 *                     Masks are unique, so the lists depend on no cut; rank 0 is lsspa_cv_best's winner and the list
 *                     for T is a prefix of the list for T' > T.  v[k][r] has the bits of lsspa_debug_cv_values for
 *                     masks[k][r]; v_fold [p+1][T][K]: the listed models' per-fold values by that same device code
 *                     (NaN past count[k]).  include, steps, info [K] as in lsspa_cv_best.  LSSPA_ERR_ARG: include
 *                     beyond p, T outside 1 .. 16, steps < 0.  Two calls agree bitwise.
 *   lsspa_cv_timing : kernel ms of the load's Gram side (weights, Gram, sums, finalise), of the last enumeration's
 *                     launches, its longest launch and their number (any pointer may be NULL)
 *   lsspa_cv_get_problem   : test hook -- fold problem f as the device computed it (G, H [p][p], g, h [p], the pooled
 *                     1 / ||y||^2; any pointer may be NULL)
 *   lsspa_debug_cv_values  : test hook -- v[i] = v_cv(masks[i]) and, unless NULL, v_fold[i][f] = v_f(masks[i]) by
 *                     lsspa_cv_best's own device code.  A failed pivot is no error here: the value is what came out.
 *   lsspa_debug_cv_plan    : host only, no context, no GPU -- lsspa_cv_best's units, high subsets per unit, steps of a
 *                     unit per launch (each K fold evaluations: 2^20 / (units K), at least 1), launches, LDS bytes of
 *                     a workgroup, its threads, 0, 0.  p outside 1 .. 32 or K outside 2 .. 32 is LSSPA_ERR_ARG.
 *   lsspa_debug_cv_top_plan: host only, no context, no GPU -- lsspa_cv_top's units, high subsets per unit, steps of a
 *                     unit per launch and launches (lsspa_debug_cv_plan's), LDS bytes of a workgroup at this T (the
 *                     static part and 20 lists of 12 T + 4 bytes), its threads, the sizes one unit can meet and the
 *                     bytes of the table (units (p + 1) (12 T + 4), lsspa_debug_subsets_top_plan's).  p outside
 *                     1 .. 32, K outside 2 .. 32 or T outside 1 .. 16 is LSSPA_ERR_ARG.
 * LSSPA_ERR_STATE before a load.  Groups of columns: the next block.  Interactions and a bootstrap over the folds are
 * not built. */
int lsspa_cv_load(lsspa_ctx* ctx, const void* X, int64_t ld, const void* y, int64_t N, int32_t p,
                  const int32_t* fold_ids /* [N], host */, int32_t K, double reg, int32_t dtype, int32_t location);
int lsspa_cv_shapley(lsspa_ctx* ctx, double* phi /* [p] */, double* phi_fold /* [K][p] */, double* r2_fold /* [K] */,
                     int32_t* info /* [K] */);
int lsspa_cv_best(lsspa_ctx* ctx, uint32_t include, int64_t steps, double* v /* [p+1] */, uint32_t* masks /* [p+1] */,
                  uint8_t* found /* [p+1] */, double* v_fold /* [p+1][K] */, int32_t* info /* [K] */);
int lsspa_cv_top(lsspa_ctx* ctx, uint32_t include, int32_t T, int64_t steps, double* v /* [p+1][T] */,
                 uint32_t* masks /* [p+1][T] */, int32_t* count /* [p+1] */, double* v_fold /* [p+1][T][K] */,
                 int32_t* info /* [K] */);
int lsspa_cv_timing(const lsspa_ctx* ctx, double* gram_ms, double* enum_ms, double* max_launch_ms, int64_t* launches);
int lsspa_cv_free(lsspa_ctx* ctx);
int lsspa_cv_get_problem(lsspa_ctx* ctx, int32_t f, double* G, double* g, double* H, double* h, double* inv_yy);
int lsspa_debug_cv_values(lsspa_ctx* ctx, const uint64_t* masks, int64_t n, double* v /* [n] */,
                          double* v_fold /* [n][K] or NULL */);
int lsspa_debug_cv_plan(int32_t p, int32_t K, int64_t* plan /* [8] */);
int lsspa_debug_cv_top_plan(int32_t p, int32_t K, int32_t T, int64_t* plan /* [8] */);

/* K-FOLD CROSS-VALIDATION OVER GROUPS OF COLUMNS (g <= 32 groups of p <= 64 columns, 2 <= K <= 32, fp64): the players
 * are the groups of `labels` (-1: the baseline, in every model; 0 .. g-1: the group), as in lsspa_groups_shapley, and
 * the game is u_cv(S) = sum_f u_f(S) (f ascending, fp64), u_f(S) = v_f(baseline + columns of the groups in S) what
 * lsspa_debug_group_values gives for fold problem f.  u_cv({}) is the baseline's own cross-validated value.
 *   lsspa_cv_groups_load   : lsspa_cv_load with the limit p <= 64 -- the same store, packing, weights, Gram pass and
 *                     fold problems, the same refusals with the same wording, naming 64.  One cross-validation problem
 *                     is loaded at a time: either load replaces the other.  After a load of p <= 32 columns by either
 *                     call both families work; after one of p > 32 lsspa_cv_shapley, lsspa_cv_best and
 *                     lsspa_debug_cv_values refuse with LSSPA_ERR_STATE.  lsspa_cv_get_problem, lsspa_cv_timing and
 *                     lsspa_cv_free serve both.
 *   lsspa_cv_groups_shapley: phi [g] = sum_f phi_fold[f] (f ascending), phi_fold [K][g] (row f has the bits
 *                     lsspa_groups_shapley gives for problem f: the same kernel, each fold cut into launches as that
 *                     call cuts one problem), r2_fold [K] = u_f(all groups), base_fold [K] = u_f({}), info [K].  phi sums
 *                     to sum r2_fold - sum base_fold.  Labels, limits and refusals are lsspa_groups_shapley's.
 *   lsspa_cv_groups_best   : lsspa_groups_best by u_cv: u [g+1], masks (the caller's numbering: bit k = label k), found
 *                     -- size 0 is the baseline alone; the larger u_cv wins, on equal values the smaller mask, so the
 *                     result depends on no cut --, candidates: the subset's own pivots passed in EVERY fold (info [K]
 *                     says which fold failed).  u[k] has the bits of lsspa_debug_cv_group_values for masks[k]; u_fold
 *                     [g+1][K]: the winner's per-fold values (NaN where found[k] = 0).  steps as in lsspa_cv_best.
 *   lsspa_debug_cv_group_values: test hook -- u[i] = u_cv(masks[i]) and, unless NULL, u_fold[i][f] = u_f(masks[i]) by
 *                     lsspa_cv_groups_best's own device code.  A failed pivot is no error here.
 *   lsspa_debug_cv_groups_plan : host only -- lsspa_debug_groups_best_plan's gl, gh, ql, nb, units and per, then
 *                     lsspa_cv_groups_best's steps of a unit per launch (each K fold evaluations: the one-problem
 *                     launch bound / (units K), at least 1, at most per), its launches, the LDS bytes of a workgroup,
 *                     its threads (256), the LDS bytes of lsspa_groups_best's workgroup and that launch bound.  Labels
 *                     the library refuses, p > 64, g > 32 or K outside 2 .. 32: LSSPA_ERR_ARG.
 *   lsspa_cv_groups_top    : lsspa_groups_top by u_cv: per size k = 0 .. g the T best sets of groups (1 <= T <= 16), best
 *                     first, in lsspa_cv_groups_best's order and over its candidates, whose sum is also above -inf (so
 *                     never NaN).  u [g+1][T], masks [g+1][T] (the caller's numbering), count [g+1] = min(T, candidates
 *                     of size k); NaN / 0 past count[k].  Masks are unique, so the lists depend on no cut; rank 0 is
 *                     lsspa_cv_groups_best's winner and the list for T is a prefix of the list for T' > T.  u[k][r] has
 *                     the bits of lsspa_debug_cv_group_values for masks[k][r]; u_fold [g+1][T][K]: the listed models'
 *                     per-fold values by that same device code (NaN past count[k]).  The cut into units, steps and
 *                     launches is lsspa_cv_groups_best's; steps, info [K] as there.  Refusals, in this order and before
 *                     any launch (the loaded folds stay usable): nothing loaded (LSSPA_ERR_STATE), a NULL pointer, the
 *                     labels (lsspa_groups_shapley's messages), T outside 1 .. 16, steps < 0 (LSSPA_ERR_ARG).  No
 *                     floating-point atomics: two calls agree bitwise.
 *   lsspa_debug_cv_groups_top_plan: host only, no context, no GPU -- lsspa_debug_cv_groups_plan's first eight entries
 *                     (gl, gh, ql, nb, units, per, steps, launches), then the LDS bytes of a workgroup of
 *                     lsspa_cv_groups_top's kernel (the same for every K and T), its threads (256), the sizes one unit
 *                     can hold (min(g, popc(per - 1) + gl) + 1) and the bytes of the table (units (g + 1) (12 T + 4)).
 *                     Labels the library refuses, p > 64, g > 32, K outside 2 .. 32 or T outside 1 .. 16:
 *                     LSSPA_ERR_ARG.
 * Interactions and a bootstrap over the folds are not built. */
int lsspa_cv_groups_load(lsspa_ctx* ctx, const void* X, int64_t ld, const void* y, int64_t N, int32_t p,
                         const int32_t* fold_ids /* [N], host */, int32_t K, double reg, int32_t dtype,
                         int32_t location);
int lsspa_cv_groups_shapley(lsspa_ctx* ctx, const int32_t* labels /* [p] */, int32_t g, double* phi /* [g] */,
                            double* phi_fold /* [K][g] */, double* r2_fold /* [K] */, double* base_fold /* [K] */,
                            int32_t* info /* [K] */);
int lsspa_cv_groups_best(lsspa_ctx* ctx, const int32_t* labels /* [p] */, int32_t g, int64_t steps,
                         double* u /* [g+1] */, uint32_t* masks /* [g+1] */, uint8_t* found /* [g+1] */,
                         double* u_fold /* [g+1][K] */, int32_t* info /* [K] */);
int lsspa_debug_cv_group_values(lsspa_ctx* ctx, const int32_t* labels /* [p] */, int32_t g, const uint64_t* masks,
                                int64_t n, double* u /* [n] */, double* u_fold /* [n][K] or NULL */);
int lsspa_debug_cv_groups_plan(const int32_t* labels /* [p] */, int32_t p, int32_t g, int32_t K,
                               int64_t* plan /* [12] */);
int lsspa_cv_groups_top(lsspa_ctx* ctx, const int32_t* labels /* [p] */, int32_t g, int32_t T, int64_t steps,
                        double* u /* [g+1][T] */, uint32_t* masks /* [g+1][T] */, int32_t* count /* [g+1] */,
                        double* u_fold /* [g+1][T][K] */, int32_t* info /* [K] */);
int lsspa_debug_cv_groups_top_plan(const int32_t* labels /* [p] */, int32_t p, int32_t g, int32_t K, int32_t T,
                                   int64_t* plan /* [12] */);

/* The RIDGE PATH of the K-fold CV attribution: lsspa_cv_shapley / lsspa_cv_groups_shapley for L ridge values on one
 * load.  reg enters a fold problem only as + reg on the diagonal of G_f, and the load keeps the per-fold Grams: the
 * L K fold problems are written from them on the device and enumerated as replicates of shared grids, a block of ridge
 * values at a time.  The load's own reg plays no part, and the loaded fold problems are not overwritten: the path has
 * buffers of its own.
 *   lsspa_cv_path_shapley : after lsspa_cv_load (or lsspa_cv_groups_load of p <= 32 columns).  regs [L] on the host,
 *                     1 <= L <= 256, every value finite and >= 0.  Row l of phi [L][p], phi_fold [L][K][p], r2_fold
 *                     [L][K] and info [L][K] is what lsspa_cv_shapley returns after a load of the same rows with
 *                     reg = regs[l].
 *   lsspa_cv_path_groups_shapley : the same after either load over the groups of labels / g (lsspa_cv_groups_shapley's
 *                     limits and messages), with base_fold [L][K].
 *   GUARANTEE: row l of every output has exactly the bits that lsspa_cv_shapley (lsspa_cv_groups_shapley) returns after
 *                     a load of the same rows with reg = regs[l], whatever L, block and the position of l in regs:
 *                     G_{l,f} is formed by the load's expressions in the load's order, a problem is cut into launches
 *                     as those calls cut a fold, and a replicate's result does not depend on the replicates beside it.
 *                     After the call lsspa_cv_shapley and every other call on the loaded folds still answer for the
 *                     load's own reg, bit for bit.  No floating-point atomics: two calls agree bitwise.
 *   block           : 0: as many ridge values a block as keep its problems within 64 MiB; > 0: that many (test hook:
 *                     the result does not depend on it).  As many of a block's replicates share a launch as the bound
 *                     of lsspa_subsets_shapley (2^20 subsets a launch) or lsspa_groups_shapley leaves.
 *   Refusals, in this order and before any launch (the loaded folds stay usable): nothing loaded, and for the column
 *                     call a load of more than 32 columns (LSSPA_ERR_STATE); a NULL pointer, L outside 1 .. 256,
 *                     block < 0, a ridge value that is negative or not finite (the message names it), the labels
 *                     (LSSPA_ERR_ARG).
 *   lsspa_cv_timing afterwards reports the path's enumeration launches; nothing else of the context changes.
 *   lsspa_debug_cv_path_plan, lsspa_debug_cv_path_groups_plan : host only, no context, no GPU.  plan [8] = units, per,
 *                     steps of a launch (one problem's cut), ridge values a block, blocks, replicates of a launch of a
 *                     full block, enumeration launches of the L values, and the bound replicates x units x steps stays
 *                     within; the grouped plan [12] has gl, gh, ql, nb in front of them.  A p, K, L, block or labels
 *                     that the calls refuse: LSSPA_ERR_ARG.
 * Measured on one MI355X (tools/cv_path_time.py, on top of commit 421be8d; N = 10^4, K = 5, L = 32): the path's
 * enumeration launches against 32 x lsspa_cv_shapley's take 0.28 x at p = 12, 0.88 x at p = 16, 0.965 x at p = 20,
 * 0.95 x at (g, p) = (12, 64) and 0.995 x at (16, 48); the whole ls_spa_cv_path call against the loop of 32 ls_spa_cv
 * calls 0.19 x, 0.30 x, 0.65 x, 0.62 x and 0.80 x (DESIGN.md has the tables).
 * Not built: a path of the selection and top-list calls (L calls on re-finalised folds would serve them). */
int lsspa_cv_path_shapley(lsspa_ctx* ctx, const double* regs /* [L] host */, int32_t L, int32_t block,
                          double* phi /* [L][p] */, double* phi_fold /* [L][K][p] */, double* r2_fold /* [L][K] */,
                          int32_t* info /* [L][K] */);
int lsspa_cv_path_groups_shapley(lsspa_ctx* ctx, const int32_t* labels /* [p] */, int32_t g,
                                 const double* regs /* [L] host */, int32_t L, int32_t block, double* phi /* [L][g] */,
                                 double* phi_fold /* [L][K][g] */, double* r2_fold /* [L][K] */,
                                 double* base_fold /* [L][K] */, int32_t* info /* [L][K] */);
int lsspa_debug_cv_path_plan(int32_t p, int32_t K, int32_t L, int32_t block, int64_t* plan /* [8] */);
int lsspa_debug_cv_path_groups_plan(const int32_t* labels /* [p] */, int32_t p, int32_t g, int32_t K, int32_t L,
                                    int32_t block, int64_t* plan /* [12] */);

/* Exact attribution of MANY RESPONSES at once (p <= 32): one design matrix, m targets.  Row r of phi is what
 * lsspa_subsets_shapley gives for response r alone (to rounding: ~1e-13), but the rows of X are reduced once and the
 * 2^p subsets are enumerated once for every 8 responses: a wave sweeps a high subset's pivots out of [G | g_r ...] with
 * eight right-hand sides, and only the two 6-long solves and the quadratic form are per response (csrc/k_multi.hip).
 * One Gram pass per side over Z = [X | Y], p + m columns, gives
 *   G = S_tr[:p,:p] / N + reg I,  g_r = S_tr[:p,p+r] / N,  H = S_te[:p,:p],  h_r = S_te[:p,p+r],  ||y_r||^2 = S_te[p+r][p+r];
 * H is always a Gram (M < p works).  fp64 throughout.
 *   lsspa_multi_load        : X [N][ld], Y [N][ldy] (m columns used) of both sides, dtype and location as lsspa_reduce's.
 *                     p > 64, m < 1 or p + m > 32767 is LSSPA_ERR_ARG naming the limit; so is a column of Y_test that
 *                     is identically zero (or NaN), which lsspa_reduce refuses for one y.  33 <= p <= 64 loads for
 *                     lsspa_multi_groups_shapley alone: lsspa_multi_shapley and lsspa_debug_multi_values then refuse
 *                     with LSSPA_ERR_ARG naming p <= 32.  Both sides are on the device
 *                     whole for the length of the call.  The loaded problem, the running statistics and the state of
 *                     lsspa_subsets_*, lsspa_groups_* and lsspa_boot_* are not touched, now or by any call below.
 *   lsspa_multi_set_reduced : the same from the Gram form (host): G, H [p][p], g, h [m][p], yy [m].
 *   lsspa_multi_shapley     : responses first .. first + count - 1 into phi [count][p] (out of range: LSSPA_ERR_ARG).
 *                     block: responses enumerated together, 0 = as many as 256 MB of partial table hold (whole chunks
 *                     of 8), a larger request is cut to that.  info: one word -- G is shared, so a failed pivot
 *                     (LSSPA_INFO_NOT_PD) concerns every response.  A response's bits depend on G, H and its own g, h,
 *                     yy alone: not on its place among the responses, on the others, on block or on first / count, and
 *                     two calls agree bitwise (no floating-point atomics, sums in a fixed order, a unit's high subsets
 *                     cut into launches by p alone).  Launches are bounded as lsspa_subsets_shapley's.
 *   lsspa_multi_get_gram    : the reduced form back (any pointer may be NULL).
 *   lsspa_multi_timing      : device ms of the last load's two Gram passes and of the last lsspa_multi_shapley's
 *                     enumeration launches, its longest launch and their number (any pointer may be NULL).
 *   lsspa_multi_free        : frees the responses and the buffers.
 *   lsspa_debug_multi_values : test hook -- v [n][m], v[i][r] = v_r(masks[i]) (bit j = feature j; masks < 2^p) by the
 *                     enumeration's own device code; a failed pivot is LSSPA_ERR_STATE.
 *   lsspa_multi_groups_shapley : the same over GROUPS of columns (g <= 32 groups over p <= 64 columns, labels as
 *                     lsspa_groups_shapley takes them: -1 the always-included baseline, 0 .. g-1 the groups; what is
 *                     wrong with them comes back in the LSSPA_ERR_ARG message).  phi [count][g] in label numbering: row r
 *                     is what lsspa_groups_shapley gives for response r alone (to rounding), and sums to the response's
 *                     R^2 minus that of its baseline.  The enumeration of csrc/k_groups.hip with eight right-hand sides
 *                     carried through one Gauss-Jordan elimination of a high subset's pivots (csrc/k_multi_groups.hip):
 *                     the elimination, H E and E^T H E are formed once for a chunk of 8 responses.  first, count,
 *                     block, the 256 MB budget, info and the bitwise independence are lsspa_multi_shapley's (a unit's
 *                     high subsets are cut into launches by the layout alone); launches are bounded as
 *                     lsspa_groups_shapley's.  lsspa_multi_timing afterwards reports this call's enumeration.
 *   lsspa_debug_multi_group_values : test hook -- u [n][m], u[i][r] = u_r(masks[i]) (bit k = label k; a mask at or beyond
 *                     2^g is LSSPA_ERR_ARG) by that enumeration's own device code; a failed pivot is LSSPA_ERR_STATE.
 * LSSPA_ERR_STATE before a load; LSSPA_ERR_NOMEM when device memory runs out.
 * Measured on one MI355X (tools/multi_time.py, on top of commit 5f361f6): the enumeration costs 1.36 ms a response at
 * p = 24 and 25.4 ms at p = 28 against lsspa_subsets_shapley's 4.6 - 4.7 ms and 87.1 ms (3.4 x), 0.0081 ms against
 * 0.038 ms at p = 16 with m = 64 (4.7 x); the longest launch 14.7 ms at p = 28 (DESIGN.md has the tables).
 * lsspa_multi_groups_shapley (tools/multi_groups_time.py, on top of commit 2f04542, m = 64): the enumeration costs
 * 0.0377 ms a response at g = 12, p = 64 against lsspa_groups_shapley's 0.322 ms (ratio 0.117), 0.190 against 1.353 ms
 * at g = 16, p = 48 (0.141), 1.001 against 6.39 ms at g = 20, p = 60 (0.157; the same at m = 8); the whole call of the
 * Python driver against the loop of m one-response calls 19.9 x, 11.1 x and 7.3 x (5.8 x at m = 8); the longest launch
 * 1.5 ms. */
int lsspa_multi_load(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* Y_train, int64_t ldy_train,
                     int64_t N, const void* X_test, int64_t ld_test, const void* Y_test, int64_t ldy_test, int64_t M,
                     int32_t p, int32_t m, double reg, int32_t dtype, int32_t location);
int lsspa_multi_set_reduced(lsspa_ctx* ctx, int32_t p, int32_t m, const double* G /* [p][p] */,
                            const double* g /* [m][p] */, const double* H /* [p][p] */, const double* h /* [m][p] */,
                            const double* yy /* [m] */);
int lsspa_multi_shapley(lsspa_ctx* ctx, int64_t first, int64_t count, int64_t block, double* phi /* [count][p] */,
                        int32_t* info);
int lsspa_multi_groups_shapley(lsspa_ctx* ctx, const int32_t* labels /* [p] */, int32_t g, int64_t first, int64_t count,
                               int64_t block, double* phi /* [count][g] */, int32_t* info);
int lsspa_multi_get_gram(lsspa_ctx* ctx, double* G, double* g, double* H, double* h, double* yy);
int lsspa_multi_timing(const lsspa_ctx* ctx, double* gram_ms, double* enum_ms, double* max_launch_ms,
                       int64_t* launches);
int lsspa_multi_free(lsspa_ctx* ctx);
int lsspa_debug_multi_values(lsspa_ctx* ctx, const uint64_t* masks, int64_t n, double* v /* [n][m] */);
int lsspa_debug_multi_group_values(lsspa_ctx* ctx, const int32_t* labels /* [p] */, int32_t g, const uint64_t* masks,
                                   int64_t n, double* u /* [n][m] */);

/* PERMUTATION TEST of the exact attribution (p <= 32; over groups g <= 32, p <= 64): the null distribution of phi and R^2
 * when y is exchangeable with respect to the rows of X.  Replicate r permutes y_train by pi_r and y_test by an
 * independent pi'_r; G, H and ||y_test||^2 do not change, only g_r = X^T y[pi_r] / N and h_r = X_test^T y_test[pi'_r]
 * do.  The rows of both sides stay on the device; for a block of replicates one fp64-MFMA pass per side gathers y
 * through the block's index rows (csrc/k_perm.hip), a fixed-order sum over the row slices writes g_r, h_r into response
 * slots, and the enumerations of lsspa_multi_shapley / lsspa_multi_groups_shapley re-attribute eight replicates a sweep.
 * The state is its own: the loaded problem, the running statistics and the state of lsspa_subsets_*, lsspa_groups_*,
 * lsspa_boot_*, lsspa_multi_* and lsspa_multi_lift_* are not touched by any call below.  fp64 throughout.
 * pi for (seed, r, side s in {0 train, 1 test}, n) is a pure function of those four: Fisher-Yates on a[i] = i, for
 * t = n - 1 down to 1 swap a[t] and a[j], j = (uint64(word) (t + 1)) >> 32, word = word t % 4 of Philox4x32-10 with key =
 * the 64-bit seed and counter = (t / 4, 2 + s, r low, r high) (the bootstrap's counters are (., s, ., .)); y_pi[i] =
 * y[a[i]].  Relative bias at most n / 2^32.
 *   lsspa_perm_load     : X [N][ld], y [N] of both sides, dtype and location as lsspa_reduce's; one Gram pass per side over
 *                     [X | y] gives G, H, the observed g, h and ||y_test||^2 (lsspa_multi_load with m = 1).  p > 64, N or
 *                     M outside 1 .. 2^31 - 1 or a y_test that is identically zero (or NaN) is LSSPA_ERR_ARG.
 *   lsspa_perm_run      : replicates first .. first + R - 1 into phi [R][d], d = p (labels NULL; p > 32 is then
 *                     LSSPA_ERR_ARG naming the limit) or d = g (labels [p] as lsspa_groups_shapley takes them).  sides:
 *                     bit 0 permutes the training side, bit 1 the test side; a side that is not permuted keeps its
 *                     observed g or h.  gperm / hperm (may be NULL): g_r, h_r [R][p].  block: replicates a pass, 0 = as
 *                     many as 256 MB hold of index rows (two sides, two buffers: 8 (N + M) bytes a replicate) and
 *                     partial sums, at most 1024; a larger request is cut to that.  The next block's index rows are
 *                     drawn by up to 16 threads of the library into pinned memory and uploaded while the GPU works on
 *                     the current one.  info: one word -- G is shared, so LSSPA_INFO_NOT_PD concerns every replicate.
 *                     A replicate's bits depend on (seed, its number) and the data alone: not on R, first, block or the
 *                     labels (gperm, hperm), and two calls agree bitwise (row slices by the row count alone, sums in a
 *                     fixed order, no floating-point atomics).
 *   lsspa_perm_observed : the identity permutation -- the observed g, h -- through the same enumeration: phi [d].
 *   lsspa_perm_get_gram : G, H [p][p], g, h [p], yy [1] of the load (any pointer may be NULL).
 *   lsspa_perm_timing   : ms of the last run: drawing and uploading the index rows (host time of the library's threads,
 *                     hidden behind the GPU from the second block on), the X^T y kernels and the enumeration (device).
 *   lsspa_perm_free     : frees the rows and every buffer.
 *   lsspa_debug_perm_indices : out [n] = a of (seed, r, side, n) above; host only, needs no context and no GPU.
 *   lsspa_debug_perm_plan    : host only -- plan10 = {block, blocks, rows per slice train / test, slices train / test,
 *                     16-column blocks of X, index row stride train / test, bytes a replicate}.  A slice is at least 256
 *                     rows, a multiple of 16, at most 128 of them a side.
 * LSSPA_ERR_STATE before a load; LSSPA_ERR_NOMEM when device or pinned memory runs out. */
int lsspa_perm_load(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* y_train, int64_t N,
                    const void* X_test, int64_t ld_test, const void* y_test, int64_t M, int32_t p, double reg,
                    int32_t dtype, int32_t location);
int lsspa_perm_run(lsspa_ctx* ctx, const int32_t* labels /* NULL or [p] */, int32_t g, int64_t R, uint64_t seed,
                   int64_t first, int32_t sides, int64_t block, double* phi /* [R][d] */, double* gperm /* [R][p] or NULL */,
                   double* hperm /* [R][p] or NULL */, int32_t* info);
int lsspa_perm_observed(lsspa_ctx* ctx, const int32_t* labels /* NULL or [p] */, int32_t g, double* phi /* [d] */,
                        int32_t* info);
int lsspa_perm_get_gram(lsspa_ctx* ctx, double* G, double* g, double* H, double* h, double* yy);
int lsspa_perm_timing(const lsspa_ctx* ctx, double* draw_ms, double* upload_ms, double* xty_ms, double* enum_ms);
int lsspa_perm_free(lsspa_ctx* ctx);
int lsspa_debug_perm_indices(uint64_t seed, uint64_t r, int32_t side, int64_t n, uint32_t* out /* [n] */);
int lsspa_debug_perm_plan(int64_t R, int64_t N, int64_t M, int32_t p, int64_t block, int64_t* plan10);

/* SAMPLED attribution of MANY RESPONSES on one design matrix (p <= 104): the lift vectors of m targets for the same
 * orderings.  Of an ordering's work the two factorisations G_pi = L L^T, H_pi = L_t L_t^T and V = L^-1 L_t are O(p^3)
 * and the same for every response; only z_r = L^-1 g_r[pi], y~_r = L_t^-1 h_r[pi] and the lift scan over V are O(p^2)
 * per response.  A workgroup of csrc/k_small_multi.hip carries 8 responses as 8 augmented rows of the two work
 * matrices (both resident in LDS) through one gather, one pair of factorisations and one V solve; the grid is
 * orderings x chunks of 8 responses.  The reduced form is lsspa_multi_load's.  fp64 throughout.
 *   lsspa_multi_lift_load   : arguments and the one Gram pass per side over [X | Y] as lsspa_multi_load's.  Limits:
 *                     1 <= p <= LSSPA_MULTI_LIFT_MAX_P, m >= 1, p + m <= 32767, and M >= p (H must have a Cholesky
 *                     factor); a column of Y_test that is identically zero (or NaN) is refused.  Each refusal is
 *                     LSSPA_ERR_ARG naming the limit.  Clears the running statistics and the info word.  The loaded
 *                     problem, the sampling path's statistics and the state of lsspa_subsets_*, lsspa_groups_*,
 *                     lsspa_boot_* and lsspa_multi_* are not touched, now or by any call below.
 *   lsspa_multi_lift_set_reduced : the same from the Gram form (host): G, H [p][p], g, h [m][p], yy [m].
 *   lsspa_multi_lift_batch  : perms [B][p], every row a permutation of 0 .. p-1 (else LSSPA_ERR_ARG).  Sample s is
 *                     ordering s, with antithetical != 0 the mean of ordering s and its reverse.  lifts_out [B][m][p]
 *                     (may be NULL): lifts_out[s][r][j] = the lift of feature j for response r in sample s.
 *                     accumulate != 0 folds the batch into the running (n, mean, M2) per (response, feature): Welford
 *                     over the batch in sample order, one Chan merge into the state, no atomics.  The batch is cut into
 *                     launches of whole samples (at most 2^16 workgroups and 256 MB of lift vectors a launch, a cut that
 *                     depends on B, m and p alone).  Returns when the batch is done.
 *   lsspa_multi_lift_set_players : GROUPS of columns as the players, as lsspa_set_players names them: labels [p], -1 the
 *                     baseline (the columns of every model), 0 .. g-1 the groups, each with a column at least (else
 *                     LSSPA_ERR_ARG saying what is wrong).  labels = NULL, g = 0 clears the map.  Setting or clearing
 *                     resets (n, mean, M2) and the info word; a new load, lsspa_multi_lift_set_reduced and
 *                     lsspa_multi_lift_free drop the map.  The map is this path's alone: lsspa_set_players' map, the
 *                     loaded problem and the state of lsspa_multi_* are not touched.  While a map is set,
 *                     lsspa_multi_lift_batch takes perms [B][g], every row a permutation of 0 .. g-1, and lifts_out is
 *                     [B][m][g]: lifts_out[s][r][k] = the summed lifts of group k's columns for response r when the
 *                     group ordering is expanded to a column ordering with the baseline first and every group's columns
 *                     contiguous and ascending; with antithetical != 0 the mean of that and of the expansion of the
 *                     reversed group ordering (the baseline stays first).  The rows are expanded on the host; the kernel
 *                     folds a response's p lifts to g in LDS -- one thread a group adds its columns in ascending order from
 *                     0.0, no atomics in the fold -- and the pair's two workgroups each add half their group lift into the
 *                     zeroed destination.  A group lift therefore has exactly the bits of that fold over the lifts_out
 *                     of the call WITHOUT a map, antithetical = 0, on the same expanded rows (then 0.5 (a + b) for a
 *                     pair), and the contract below holds with g for p.  The cut into launches depends on B, m, p and g
 *                     alone.  lsspa_multi_lift_get returns [m][g].
 *   lsspa_multi_lift_get    : n, mean [m][p], m2 [m][p] (any pointer may be NULL); waits for work in flight.
 *   lsspa_multi_lift_reset  : n = 0, the info word cleared.
 *   lsspa_multi_lift_get_gram : the reduced form back, as lsspa_multi_get_gram.
 *   lsspa_multi_lift_info   : one word -- G and H are shared, so a failed pivot (LSSPA_INFO_NOT_PD) concerns every
 *                     response.  Only the pivots j < p of either matrix count, with the relative test 16 p eps; the
 *                     augmented rows' own pivots never raise it (a response in the span of X is as good as any other).
 *   lsspa_multi_lift_timing : device ms of the last load's two Gram passes, of the last batch's lift launches and of its
 *                     statistics launches (any pointer may be NULL).
 *   lsspa_multi_lift_free   : frees the responses, the statistics and the buffers.
 * LSSPA_ERR_STATE before a load (lsspa_multi_lift_free and lsspa_multi_lift_timing excepted: freeing nothing is not an
 * error, as for lsspa_multi_free); LSSPA_ERR_NOMEM when device memory runs out.
 * Contract: two calls agree bitwise (the antithetical pair's two terms are added into a zeroed destination, a sum that
 * commutes).  The bits of response r's lifts depend on G, H, the ordering, its own g_r, h_r, yy_r, p and its slot
 * r mod 8 -- not on the other responses' values, on m beyond the slot, on B, on the other orderings of the batch or on
 * how a batch is cut.  Independence of the slot itself is NOT promised: the augmented rows may straddle a 16-row block
 * edge and then take another, equally accurate, route; across slots the results agree to the accuracy of the
 * one-response path (tests/test_gpu_multi_sampled.py).
 * Measured on one MI355X (tools/multi_sampled_time.py, on top of commit cd86a46; N = M = 10^4, 256 antithetical samples a
 * batch): a batch costs 0.0092 ms a response at p = 40, m = 8 and 0.0085 ms at m = 64 against lsspa_lift_batch's 0.029 ms
 * on one response (ratios 0.31 and 0.30), 0.0221 and 0.0208 ms at p = 100 against 0.064 ms (0.34 and 0.33); the whole call
 * of the Python driver against the loop of m one-response calls 8.7 x and 49 x at p = 40, 13.5 x and 60 x at p = 100
 * (DESIGN.md has the tables). */
#define LSSPA_MULTI_LIFT_MAX_P 104
int lsspa_multi_lift_load(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* Y_train, int64_t ldy_train,
                          int64_t N, const void* X_test, int64_t ld_test, const void* Y_test, int64_t ldy_test,
                          int64_t M, int32_t p, int32_t m, double reg, int32_t dtype, int32_t location);
int lsspa_multi_lift_set_reduced(lsspa_ctx* ctx, int32_t p, int32_t m, const double* G /* [p][p] */,
                                 const double* g /* [m][p] */, const double* H /* [p][p] */,
                                 const double* h /* [m][p] */, const double* yy /* [m] */);
int lsspa_multi_lift_set_players(lsspa_ctx* ctx, const int32_t* labels /* [p] or NULL */, int32_t g);
int lsspa_multi_lift_batch(lsspa_ctx* ctx, const int32_t* perms /* [B][p] */, int64_t B, int32_t antithetical,
                           double* lifts_out /* [B][m][p] or NULL */, int32_t accumulate);
int lsspa_multi_lift_get(lsspa_ctx* ctx, int64_t* n, double* mean /* [m][p] */, double* m2 /* [m][p] */);
int lsspa_multi_lift_reset(lsspa_ctx* ctx);
int lsspa_multi_lift_get_gram(lsspa_ctx* ctx, double* G, double* g, double* H, double* h, double* yy);
int lsspa_multi_lift_info(lsspa_ctx* ctx, int32_t* info);
int lsspa_multi_lift_timing(const lsspa_ctx* ctx, double* gram_ms, double* batch_ms, double* stats_ms);
int lsspa_multi_lift_free(lsspa_ctx* ctx);

/* SAMPLED attribution of the K-FOLD CROSS-VALIDATED R^2 (p <= 127): the game of lsspa_cv_load -- fold problem f trained
 * on the other folds' rows and tested on fold f, every fold divided by the pooled ||y||^2 (the definition above
 * lsspa_cv_load) -- estimated from sampled orderings.  A sample's lift vector is sum_f lift_f(pi) for ONE ordering pi
 * shared by all folds.  One launch of csrc/k_small.hip's fold-problem instantiations runs a cut of the batch with the
 * grid (orderings, K): blockIdx.y selects the fold problem, addressed at one stride; the ordering's p lifts are stored to
 * raw[ordering][fold][p] by plain stores.  cv_lift_fold_kernel (csrc/k_cv.hip) takes raw to batch[sample][K + 1][d], rows
 * 0 .. K-1 the folds and row K their sum in ascending fold order, and launch_multi_lift_stats folds that into the running
 * (n, mean, M2).  fp64 throughout, no atomics anywhere.  The family has state of its own: the loaded problem, lsspa_cv_*,
 * lsspa_multi_lift_* and every other store are not touched by any call below.
 *   lsspa_cv_lift_load  : arguments as lsspa_cv_load's.  Limits: 1 <= p <= LSSPA_CV_LIFT_MAX_P, 2 <= K <= 32, fold labels
 *                     0 .. K-1, no empty fold, every fold at least p rows (H_f must have a Cholesky factor; the message
 *                     names the fold and its size), y not identically zero; each refusal is LSSPA_ERR_ARG naming the
 *                     limit, before any GPU work.  The rows [X | y] are packed SORTED BY FOLD, stable in row order, so that
 *                     fold f is a contiguous slice; the Gram reduction of lsspa_reduce (any width) runs once per slice
 *                     for S_f, and the K problems are finalised by lsspa_cv_load's expressions in its order:
 *                     G_f = (sum_{j != f} S_j) / (N - n_f) + reg I with j ascending (no "total minus S_f"), H_f = S_f,
 *                     one pooled 1 / ||y||^2.  The two loads reduce the rows in different orders: their problems agree
 *                     to round-off, not bitwise.  Clears the statistics, the info words and a player map.
 *   lsspa_cv_lift_set_players : groups of columns as the players; meaning and reset rules are those of
 *                     lsspa_multi_lift_set_players (labels [p], -1 the baseline, 0 .. g-1; NULL, 0 clears; setting or
 *                     clearing resets the statistics and the info words; a load and lsspa_cv_lift_free drop the map).
 *                     With a map d = g, else d = p.
 *   lsspa_cv_lift_batch : perms [B][d], every row a permutation of 0 .. d-1 (else LSSPA_ERR_ARG).  Sample s is ordering
 *                     s, with antithetical != 0 that ordering and its reverse (with a map: the reversed group ordering,
 *                     the baseline first in both; rows are expanded on the host exactly as lsspa_multi_lift_batch's).
 *                     fold_lifts_out [B][K][d] and lifts_out [B][d] may be NULL.  accumulate != 0 folds the batch into
 *                     the running statistics.  The batch is cut into launches of whole samples: at most 2^16 workgroups
 *                     (2^13 of the LDS-resident form, which runs one workgroup a compute unit) and 256 MB of raw lifts a
 *                     launch, a function of B, K, p and d alone.  Returns when the batch is done.
 *   lsspa_cv_lift_get   : n, mean [K + 1][d], m2 [K + 1][d] (any may be NULL): rows 0 .. K-1 the folds, row K the sum.
 *   lsspa_cv_lift_reset : n = 0, the info words cleared.
 *   lsspa_cv_lift_get_problem : G [p][p], g [p], H [p][p], h [p], inv_yy of fold problem f as the device computed it.
 *   lsspa_cv_lift_info  : info [K], bit LSSPA_INFO_NOT_PD of word f: a pivot of G_f or H_f failed the relative test
 *                     16 p eps in some ordering since the last reset.
 *   lsspa_cv_lift_timing : device ms of the last load's Gram side (pack to finalise), of the last batch's lift launches
 *                     and of its fold and statistics launches.
 *   lsspa_cv_lift_free  : frees everything of the family.
 *   lsspa_debug_cv_lift_plan : host only, no context, no GPU.  plan [8] = block rows nb = ceil((p + 1) / 16), the kernel
 *                     form (0 register-resident, 1 LDS-resident), workgroups per sample, samples per launch, launches,
 *                     LDS bytes of a workgroup, its threads, 0.  LSSPA_ERR_ARG outside the limits.
 * LSSPA_ERR_STATE before a load (lsspa_cv_lift_free and lsspa_cv_lift_timing excepted); LSSPA_ERR_NOMEM when device
 * memory runs out.
 * Contract: two calls agree bitwise.  The bits of a sample's fold lifts and of its sum depend on the fold problems, the
 * ordering, p and K only -- not on B, on the other orderings, on how a batch is cut into launches or calls, or on
 * accumulate.  lifts_out[s] has exactly the bits of the ascending fold sum ((l_0 + l_1) + l_2) + .. of
 * fold_lifts_out[s].  An antithetical sample has the bits of 0.5 * a + 0.5 * b of the two orderings run as plain
 * samples.  A group lift has the bits of the ascending-column fold (from 0.0) of the column call on the expanded rows.
 * Not built: fp32, several ranks, checkpoints, the device error estimator, the history, and a sampled CV of the
 * interaction values. */
#define LSSPA_CV_LIFT_MAX_P 127
int lsspa_cv_lift_load(lsspa_ctx* ctx, const void* X, int64_t ld, const void* y, int64_t N, int32_t p,
                       const int32_t* fold_ids /* [N] host */, int32_t K, double reg, int32_t dtype, int32_t location);
int lsspa_cv_lift_set_players(lsspa_ctx* ctx, const int32_t* labels /* [p] or NULL */, int32_t g);
int lsspa_cv_lift_batch(lsspa_ctx* ctx, const int32_t* perms /* [B][d] */, int64_t B, int32_t antithetical,
                        double* fold_lifts_out /* [B][K][d] or NULL */, double* lifts_out /* [B][d] or NULL */,
                        int32_t accumulate);
int lsspa_cv_lift_get(lsspa_ctx* ctx, int64_t* n, double* mean /* [K + 1][d] */, double* m2 /* [K + 1][d] */);
int lsspa_cv_lift_reset(lsspa_ctx* ctx);
int lsspa_cv_lift_get_problem(lsspa_ctx* ctx, int32_t f, double* G, double* g, double* H, double* h, double* inv_yy);
int lsspa_cv_lift_info(lsspa_ctx* ctx, int32_t* info /* [K] */);
int lsspa_cv_lift_timing(const lsspa_ctx* ctx, double* gram_ms, double* batch_ms, double* stats_ms);
int lsspa_cv_lift_free(lsspa_ctx* ctx);
int lsspa_debug_cv_lift_plan(int32_t p, int32_t d, int32_t K, int64_t B, int32_t antithetical, int64_t* plan /* [8] */);

/* BOOTSTRAP OF THE SAMPLED ATTRIBUTION (p <= 127): how far the attribution lsspa_small / ls_spa estimates from sampled
 * orderings moves under another draw of the rows.  The replicates are lsspa_boot_run's -- the counts rule (Philox4x32-10
 * keyed by (seed, replicate, side)), the weighted Gram pass over rows that stay on the device, its finalise -- with two
 * differences: Z = [X | y] is packed at ldz = 16 cb, cb = ceil((p + 1) / 16) <= 8, and for cb = 6 .. 8 the Gram pass
 * runs in a WIDE form in which the four waves of a workgroup share the rows and the replicate and divide the block pairs
 * bi <= bj among themselves (csrc/k_boot.hip); and a replicate is not enumerated but run through ONE SET OF ORDERINGS
 * that all replicates and the point problem share (common random numbers): the fold-problem instantiations of
 * csrc/k_small.hip with the grid (orderings, replicates), blockIdx.y the replicate, plain stores to
 * raw[ordering][replicate][p], and boot_lift_stats_kernel's Welford / Chan merge into one (n, mean, M2) per replicate.
 * fp64 throughout, no floating-point atomics anywhere.  The family has state of its own: the loaded problem,
 * lsspa_boot_*, lsspa_cv_lift_*, lsspa_multi_lift_* and every other store are not touched by any call below.
 *   lsspa_boot_lift_load : both sides as lsspa_boot_load takes them.  Limits: 1 <= p <= LSSPA_BOOT_LIFT_MAX_P, N >= p,
 *                     M >= p, y_test not identically zero; each refusal is LSSPA_ERR_ARG naming the limit, before any
 *                     GPU work.  Drops a player map and the orderings.
 *   lsspa_boot_lift_set_players : as lsspa_cv_lift_set_players (labels [p], -1 the baseline, 0 .. g-1, any 1 <= g <= p;
 *                     NULL, 0 clears).  Setting or clearing drops the orderings.  With a map d = g, else d = p.
 *   lsspa_boot_lift_set_orderings : perms [n_samples][d], every row a permutation of 0 .. d-1 (else LSSPA_ERR_ARG),
 *                     validated on the host, expanded as lsspa_cv_lift_batch expands them (with antithetical != 0 a
 *                     sample is the ordering and its reverse; with a map the reversed group ordering, the baseline first
 *                     in both) and uploaded once.
 *   lsspa_boot_lift_run : replicates first .. first + R - 1.  w_train [R][N] / w_test [R][M]: the caller's weights of a
 *                     side (finite, >= 0, a positive sum per replicate) or NULL: the counts of (boot_seed, replicate,
 *                     side), exactly lsspa_boot_debug_counts'.  block: replicates per block, 0: as many as
 *                     BOOT_BLOCK_BYTES holds.  Out: mean [R][d], m2 [R][d] over the n_samples samples, r2 [R] of the
 *                     full model and baseline_r2 [R] (may be NULL) of the baseline's columns alone, both on the host
 *                     from the replicate's problem as the device wrote it (NaN where G has no Cholesky factor),
 *                     info [R] (bit LSSPA_INFO_NOT_PD: a pivot of G or H failed the relative test 16 p eps in some
 *                     ordering).  samples_out [R][n_samples][d] (test hook, may be NULL): every sample's entry.
 *   lsspa_boot_lift_point : the original rows, weight 1 on every row, through the same Gram pass and the same kernels
 *                     as a run of one problem: mean [d], m2 [d], r2, baseline_r2 (may be NULL), info [1],
 *                     samples_out [n_samples][d] or NULL.
 *   lsspa_boot_lift_get_problem : G [p][p], g [p], H [p][p], h [p], inv_yy of replicate r as the device writes it in a
 *                     run: the counts of (boot_seed, r, side), or the caller's weights w_train [N] / w_test [M] of that
 *                     one replicate; r < 0: the point problem (weight 1 where no weights are given).
 *   lsspa_boot_lift_debug_grams : S_train / S_test [R][c][c], c = p + 1, and wsum [R] before finalise, as
 *                     lsspa_boot_debug_grams (a side without weights gets ones); any output may be NULL.
 *   lsspa_boot_lift_timing : device ms of the last pass: counts, Gram side (to the problems), lift launches, statistics
 *                     launches; and the number of lift launches.
 *   lsspa_boot_lift_free : frees everything of the family.
 *   lsspa_debug_boot_lift_plan : host only, no context, no GPU.  plan [16] = cb, the Gram kernel form (0: one wave a
 *                     replicate set, cb <= 5; 1: wide), rows per slice train / test, slices train / test, replicates per
 *                     block, blocks, replicates per lift launch, orderings per lift launch, samples per lift launch,
 *                     sample cuts, lift launches of the run, raw bytes of the largest launch, the lift kernel form
 *                     (0 register-resident, 1 LDS-resident), bytes a replicate takes in a block.  A lift launch has at
 *                     most 2^16 workgroups (2^13 of the LDS-resident form, p + 1 > 112) and 256 MB of raw lifts.
 * LSSPA_ERR_STATE before a load or, for run and point, before the orderings are set.
 * Contract: two calls agree bitwise.  Replicate r has the same bits whatever R, first, block and the number of
 * replicates that share its launches: the row slices are a function of the side's rows alone, a workgroup computes one
 * (ordering, replicate) whole, and the cut of the samples into launches -- which the Chan merges follow, in sample order
 * -- is a function of n_samples and antithetical alone.  Its counts are lsspa_boot_debug_counts' for (boot_seed, r,
 * side).  A sample's entry has the bits lsspa_cv_lift_batch documents: 0.5 * a + 0.5 * b of a pair, the ascending-column
 * sum from 0.0 of a group.  No existing call changes.
 * Not built: fp32 work matrices, several ranks, checkpoints, the device error estimator, the history, a tolerance. */
#define LSSPA_BOOT_LIFT_MAX_P 127
int lsspa_boot_lift_load(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* y_train, int64_t N,
                         const void* X_test, int64_t ld_test, const void* y_test, int64_t M, int32_t p, double reg,
                         int32_t dtype, int32_t location);
int lsspa_boot_lift_set_players(lsspa_ctx* ctx, const int32_t* labels /* [p] or NULL */, int32_t g);
int lsspa_boot_lift_set_orderings(lsspa_ctx* ctx, const int32_t* perms /* [n_samples][d] */, int64_t n_samples,
                                  int32_t antithetical);
int lsspa_boot_lift_run(lsspa_ctx* ctx, int64_t R, uint64_t boot_seed, int64_t first, const double* w_train,
                        const double* w_test, int64_t block, double* mean /* [R][d] */, double* m2 /* [R][d] */,
                        double* r2 /* [R] */, double* baseline_r2 /* [R] or NULL */, int32_t* info /* [R] */,
                        double* samples_out /* [R][n_samples][d] or NULL */);
int lsspa_boot_lift_point(lsspa_ctx* ctx, double* mean, double* m2, double* r2, double* baseline_r2, int32_t* info,
                          double* samples_out);
int lsspa_boot_lift_get_problem(lsspa_ctx* ctx, int64_t r, uint64_t boot_seed, const double* w_train, const double* w_test,
                                double* G, double* g, double* H, double* h, double* inv_yy);
int lsspa_boot_lift_debug_grams(lsspa_ctx* ctx, int64_t R, const double* w_train, const double* w_test, double* S_train,
                                double* S_test, double* wsum);
int lsspa_boot_lift_timing(const lsspa_ctx* ctx, double* counts_ms, double* gram_ms, double* lift_ms, double* stats_ms,
                           int64_t* launches);
int lsspa_boot_lift_free(lsspa_ctx* ctx);
int lsspa_debug_boot_lift_plan(int64_t R, int64_t N, int64_t M, int32_t p, int32_t d, int64_t n_samples,
                               int32_t antithetical, int64_t block, int64_t* plan /* [16] */);

/* Element type of the per-ordering work (Cholesky factors, solves): LSSPA_F64 (default; matches the
 * reference to ~1e-15) or LSSPA_F32 (half the HBM traffic, fp32 MFMA; the Gram reduction, the lift
 * accumulation and the running statistics stay fp64).  The reference has no counterpart: it computes
 * in float64 throughout (ls_spa/ls_spa.py:309-317). */
int lsspa_set_precision(lsspa_ctx* ctx, int32_t dtype);

int lsspa_get_problem(const lsspa_ctx* ctx, int32_t* p, int32_t* m, int32_t* tri, double* y_norm_sq);
/* device -> host copies of the reduced problem; any pointer may be NULL */
int lsspa_get_gram(lsspa_ctx* ctx, double* G, double* g, double* H, double* h);

/* a7 -- replaces theta = lstsq(...) and r_squared (ls_spa/ls_spa.py:240-243): factor the
 * identity ordering, back-substitute, sum its lift vector.  info: LSSPA_INFO_* flags. */
int lsspa_full_fit(lsspa_ctx* ctx, double* theta, double* r_squared, int32_t* info);
/* the reduce_data outputs in the reference's layout: R_tr [p][p] upper triangular,
 * q_tr [p], F_te [m][p], q_te [m]  (any pointer may be NULL) */
int lsspa_get_factors(lsspa_ctx* ctx, double* R_tr, double* q_tr, double* F_te, double* q_te);

/* a2 + a3 -- replaces square_shapley over a batch of orderings and the antithetical
 * pairing (ls_spa/ls_spa.py:203-208, :256-287).  perms: host int32 [B][p].  With
 * antithetical != 0 every ordering is also evaluated reversed and the two lift vectors are
 * averaged (one sample).  lifts_out: host [B][p] or NULL.  accumulate = 1: add the batch's
 * moments about the running mean to the pending-batch buffer (a4: all-reduce it over the ranks if there are several,
 * then lsspa_stats_merge).  accumulate = 2, one GPU: fold the batch into the running statistics at once -- the effect
 * of accumulate = 1 followed by lsspa_stats_merge (ls_spa/ls_spa.py:212-216 for the whole batch), in one launch for
 * p <= 128; refused (LSSPA_ERR_STATE) while a batch is pending. */
int lsspa_lift_batch(lsspa_ctx* ctx, const int32_t* perms, int32_t B, int32_t antithetical,
                     double* lifts_out, int32_t accumulate);
/* The two halves of lsspa_lift_batch.  lsspa_lift_launch enqueues every kernel of a batch up to its lift vectors and
 * returns a ticket; nothing it does touches the running statistics.  lsspa_lift_collect folds `count` samples of the
 * ticket's batch, from sample `first` on, into the pending buffer (accumulate) and / or copies their lift vectors out
 * (count <= 0: all the rest); the parts of a batch are taken front to back.  lsspa_lift_discard drops what is left.
 * Why: the reference evaluates its stop rule after every batch_size samples (ls_spa/ls_spa.py:222-230); a batch
 * that small may fill a fraction of the GPU (16 samples per rank when 128 are dealt over 8 GPUs).  The driver
 * therefore launches several chunks of a QMC sampler's orderings as ONE batch, accumulates and checks them chunk by
 * chunk in the reference's order, and discards the chunks beyond a stop -- same results, a fuller GPU.  With two
 * lanes (lsspa_set_lanes) a second batch may be launched before the first is fully collected. */
int lsspa_lift_launch(lsspa_ctx* ctx, const int32_t* perms, int32_t B, int32_t antithetical, int32_t* ticket);
int lsspa_lift_collect(lsspa_ctx* ctx, int32_t ticket, int32_t first, int32_t count, double* lifts_out,
                       int32_t accumulate);
/* n_chunks consecutive parts of `chunk` samples each, from sample `first` on, folded one after the other: the effect of
 * n_chunks calls of lsspa_lift_collect(ticket, first + c chunk, chunk, NULL, accumulate).  With accumulate = 2 on a small
 * problem (p <= 128, chunks of up to 512 samples, at most 32 of them, one rank) the parts' statistics are ONE launch
 * (every part still merged by itself, in order: the same numbers to the last bit) -- at p = 100 a part's own launch is
 * a fifth of its step and cannot hide behind the next batch's kernel. */
int lsspa_lift_collect_chunks(lsspa_ctx* ctx, int32_t ticket, int32_t first, int32_t chunk, int32_t n_chunks,
                              int32_t accumulate);
int lsspa_lift_discard(lsspa_ctx* ctx, int32_t ticket);
/* Sampled attribution over GROUPS of columns: a player map.  labels [p] as in lsspa_groups_shapley (-1: baseline, 0 ..
 * g-1: group, none empty), any 1 <= g <= p.  From now until the next reduction, lsspa_set_reduced or
 * lsspa_set_players(ctx, NULL, 0): perms of lsspa_lift_batch / lsspa_lift_launch are [B][g] orderings of the GROUPS (each
 * row a permutation of 0 .. g-1); lifts_out, the pending buffer, running statistics, history, estimator state, result
 * slots and every other [p]-sized output of the sampling path have dimension g.  The library expands a group ordering to
 * the column ordering "baseline columns, then each group's columns (ascending) in the ordering's order", runs it through
 * the same kernels, checks the un-folded lifts against the full R^2 as ever (LSSPA_INFO_SUM) and then folds them on the
 * device: sample s, group k = mean over the sample's one or two orderings of the sum of its columns' lifts, in a fixed
 * order (two runs agree bitwise).  The mean over all g! group orderings is lsspa_groups_shapley's phi.  Antithetical: the
 * second ordering is the baseline followed by the groups in REVERSED order; with a baseline the pair runs as two unpaired
 * orderings, without one as the kernels' pair (the forward column ordering read backwards, an expansion of the reversed
 * group ordering).  Setting or clearing a map resets the running statistics and switches history and estimator off
 * (enable them again: their row stride is the sample dimension); lsspa_full_fit, lsspa_get_factors, lsspa_debug_factor,
 * the enumerations and the reduction side are untouched by it.  Refused (LSSPA_ERR_STATE) while a launched batch is
 * uncollected; bad labels are LSSPA_ERR_ARG.  With no map set every entry point behaves bit for bit as before.
 *   lsspa_debug_expand_groups : test hook, host only (no context, no GPU) -- out [B * (antithetical ? 2 : 1)][p] = the
 *                               column orderings the kernels are given for group_perms [B][g]; bad labels or a row that
 *                               is not a permutation of 0 .. g-1 is LSSPA_ERR_ARG */
int lsspa_set_players(lsspa_ctx* ctx, const int32_t* labels, int32_t g);
int lsspa_debug_expand_groups(const int32_t* labels, int32_t p, int32_t g, const int32_t* group_perms, int32_t B,
                              int32_t antithetical, int32_t* out);
/* Sampled pairwise Shapley interaction index, for any number of players d = p, or g under lsspa_set_players (the exact
 * enumerations above stop at 32).  For a uniformly random ordering pi in which a and b sit at adjacent positions k, k + 1,
 * S = {pi_0 .. pi_{k-1}} carries exactly the index's weight, so I_ab = E[v(S+a+b) - v(S+a) - v(S+b) + v(S) | a, b adjacent].
 * One SAMPLE is three orderings through the ordinary kernels -- pi, pi with positions (0,1), (2,3), .. swapped, pi with
 * positions (1,2), (3,4), .. swapped -- and yields that difference for all d - 1 adjacent pairs of pi: with b = pi_{k+1},
 * Delta_k = lift_pi[b] - lift_pi'[b], pi' the row that swaps k and k + 1.  Every row is itself a uniformly random ordering.
 *   lsspa_pairs_enable : on != 0 allocates and zeroes the pair state (the sample count, a sum of lift vectors [d] and
 *                        three d x d tables: count as int64, mean, M2); 2 <= d <= LSSPA_PAIRS_MAX_D (three tables of
 *                        134 MB there), else LSSPA_ERR_ARG.  on == 0 frees it.  A reduction, lsspa_set_reduced and
 *                        setting or clearing a player map switch the state off (the dimension changed).
 *   lsspa_pairs_batch  : perms [B][d], every row a permutation of 0 .. d-1 (else LSSPA_ERR_ARG).  Runs the 3 B rows as one
 *                        unpaired batch (group expansion, fold and the LSSPA_INFO_SUM check included), then on the device
 *                        folds every Delta into its pair's (count, mean, M2) -- Welford over the batch in sample order,
 *                        one Chan merge into the table, no atomics: two runs agree bitwise -- and adds the 3 B lift
 *                        vectors to the sum.  Takes and releases a lane itself; LSSPA_ERR_STATE while a launched batch is
 *                        uncollected or the state is off.  Running statistics, pending buffer, history, estimator state
 *                        and result slots are not touched.
 *   lsspa_pairs_get    : n_samples; phi [d] = mean of all 3 n lift vectors (an unbiased attribution: every one of them
 *                        sums to the full R^2); count, mean, m2 [d*d]: symmetric, zero diagonal; mean is the raw index
 *                        estimate of the pair, m2 the sum of squared deviations of its count values.  Any pointer may be
 *                        NULL.  Waits for work in flight.
 *   lsspa_pairs_reset  : zero the state, keep it on.
 *   lsspa_debug_expand_pairs : test hook, host only (no context) -- out [3 B][d], the rows a batch runs; a row of perms
 *                        that is not a permutation, d < 1 or B < 1 is LSSPA_ERR_ARG
 *   lsspa_debug_pairs_inject : test hook -- the pair kernels alone on given lifts [3 B][d] (host) and perms [B][d]; no
 *                        ordering is factored (the counterpart of lsspa_debug_lift_inject) */
#define LSSPA_PAIRS_MAX_D 4096
int lsspa_pairs_enable(lsspa_ctx* ctx, int32_t on);
int lsspa_pairs_batch(lsspa_ctx* ctx, const int32_t* perms /* [B][d] */, int32_t B);
int lsspa_pairs_get(lsspa_ctx* ctx, int64_t* n_samples, double* phi /* [d] */, int64_t* count /* [d*d] */,
                    double* mean /* [d*d] */, double* m2 /* [d*d] */);
int lsspa_pairs_reset(lsspa_ctx* ctx);
int lsspa_debug_expand_pairs(int32_t d, const int32_t* perms, int32_t B, int32_t* out /* [3B][d] */);
int lsspa_debug_pairs_inject(lsspa_ctx* ctx, const double* lifts /* [3B][d] */, const int32_t* perms /* [B][d] */,
                             int32_t B);
/* 1 (default): every batch runs on the context's stream, one after the other.  2: successive batches alternate
 * between two workspaces on two streams, staggered by half a batch, so that the memory-bound stages (gather, lifts)
 * and the launch tails of one batch run beside the matrix-pipe-bound stages of the other; statistics, collectives
 * and merges stay in batch order on the context's stream.  Results do not depend on the setting. */
int lsspa_set_lanes(lsspa_ctx* ctx, int32_t n);
int lsspa_get_info(lsspa_ctx* ctx, int32_t* info);
/* The same word without waiting for batches that were launched and never collected (they may still be running on a
 * lane): the bits of every batch whose samples were collected are in it.  lsspa_get_info waits for everything. */
int lsspa_get_info_collected(lsspa_ctx* ctx, int32_t* info);
/* Every ordering's lifts telescope to the R^2 of the full model (ls_spa/ls_spa.py:284-285), so every sample's lift
 * vector must sum to it.  Once lsspa_full_fit has computed that R^2, every batch is checked on the device right after
 * its lifts: a deviation beyond 1e-9 max(1, |R^2|) (fp32 per-ordering work: 1e-4) raises LSSPA_INFO_SUM -- the data a
 * kernel took from another workgroup, a tile left out, an ordering read wrong all show here.  The 1e-9 holds while the
 * smallest relative pivot L_jj^2 / G_jj that lsspa_full_fit met is at least 1e6 times the NOT_PD threshold 16 p eps;
 * below that it grows with 1 / pivot (the round-off of the Gram / Cholesky route does), up to 1e-3.  (That pivot, of
 * G's and in tri mode H's factors under the identity ordering, is taken when lsspa_full_fit is asked for r_squared,
 * together with the R^2 itself.)  This returns the largest
 * deviation of all batches since the last lsspa_stats_reset (waits for everything in flight). */
int lsspa_get_sum_deviation(lsspa_ctx* ctx, double* max_deviation);

/* a4 -- replaces merge_sample_mean / merge_sample_cov (ls_spa/ls_spa.py:103-119, :212-216).
 * The pending-batch buffer is a device fp64 array [1 + p + p*p] = [n_b, sum(l - mu), sum (l - mu)(l - mu)^T];
 * with several GPUs it is the (only) all-reduce target; lsspa_stats_merge folds it into the
 * running (n, mean, M2) by Chan's pairwise update and clears it. */
int lsspa_stats_reset(lsspa_ctx* ctx);
int lsspa_stats_pending(lsspa_ctx* ctx, void** device_ptr, int64_t* count);
int lsspa_stats_merge(lsspa_ctx* ctx);
/* n samples, mean [p], biased covariance [p][p] (may be NULL); with a player map (lsspa_set_players) p reads g here and
 * in lsspa_stats_set, lsspa_stats_pending, lsspa_history_get / _append, lsspa_error_quantiles, lsspa_error_result and
 * lsspa_error_state_get / _set */
int lsspa_stats_get(lsspa_ctx* ctx, int64_t* n, double* mean, double* cov_biased);
/* checkpoint / resume: overwrite the running statistics with (n, mean [p], biased covariance [p][p]) as
 * lsspa_stats_get returned them; the pending buffer is cleared.  (The reference keeps these in three Python
 * locals, ls_spa/ls_spa.py:190-192, and cannot resume.) */
int lsspa_stats_set(lsspa_ctx* ctx, int64_t n, const double* mean, const double* cov_biased);

/* a5 -- device-side replacement of error_estimates (ls_spa/ls_spa.py:321-341) in its thin form:
 * 1024 draws x = Xi (L - 1 mean^T) / sqrt(n (n - 1)) with L the [n][p] lift vectors of all samples so far, which
 * has the covariance C_unbiased / n the reference samples from, without any p x p factorisation.
 *   lsspa_history_enable : keep every accumulated sample's lift vector in HBM (capacity = rows allocated up front,
 *                          grown geometrically when exceeded; 0 switches the history -- and the running form below -- off
 *                          and gives a history of more than 64 MB back; smaller buffers stay for the next call).
 *                          lsspa_stats_reset / lsspa_reduce / lsspa_set_reduced empty the history.
 *   lsspa_history_get    : copy it out ([count][p], host); lifts may be NULL to query the count
 *   lsspa_history_append : push rows back in (resume)
 *   lsspa_error_draws    : xi is host fp64 [1024][ld_xi], standard normals; its first n_local columns go with this
 *                          context's n_local history rows, in order.  n_total is the sample count over all ranks
 *                          (== n_local on one GPU).  The centring uses the merged running mean.
 *   lsspa_error_buffer   : device pointer / element count of the draws, the all-reduce(SUM) target between
 *                          lsspa_error_draws and lsspa_error_quantiles when the samples are spread over ranks
 *   lsspa_error_quantiles: feature_errors [p] = 0.95-quantile of |x_a| over the draws, overall_error = the same
 *                          quantile of ||x||_2 (numpy's default linear interpolation)
 * Lifetime of host buffers: every entry point that takes a host pointer has finished reading it when it returns
 * (lsspa_error_draws and lsspa_stats_set synchronise their upload; lsspa_lift_batch copies the orderings into
 * pinned staging before it returns), so the caller may pass temporaries. */
int lsspa_history_enable(lsspa_ctx* ctx, int64_t capacity);
int lsspa_history_get(lsspa_ctx* ctx, int64_t* count, double* lifts);
int lsspa_history_append(lsspa_ctx* ctx, const double* lifts, int64_t rows);
int lsspa_error_draws(lsspa_ctx* ctx, const double* xi, int64_t ld_xi, int64_t n_local, int64_t n_total);
int lsspa_error_buffer(lsspa_ctx* ctx, void** device_ptr, int64_t* count);
int lsspa_error_quantiles(lsspa_ctx* ctx, double* feature_errors, double* overall_error);

/* a5, running form (what ls_spa(error_estimator='device') uses since round 5) -- the same estimator with a cost per
 * check that does not depend on the number of samples, and no host random numbers.  Xi[d][k], draw d of sample k, is a
 * pure function of (seed, k, d): Philox4x32-10 with key = seed and counter = (k, d / 2), Box-Muller on its four
 * output words (k_error.hip; the generator's published known-answer vectors and the normals themselves are pinned by
 * tests/philox_ref.py through lsspa_error_xi).  The context keeps D = Xi L [1024][p] and s = Xi 1 [1024] over the
 * samples folded in so far; at a check x = (D - s mean^T) / sqrt(n (n - 1)), which given the lift vectors is
 * N(0, C_unbiased / n) exactly as the reference's draws are (ls_spa/ls_spa.py:334-336), and the quantiles follow as
 * above (:337-340).  Successive checks share the columns of Xi of the samples they share (the reference redraws).
 *   lsspa_error_running_enable  : allocate and zero D, s (and a small staging of lift vectors: every sample that
 *                                 lsspa_lift_batch / _collect accumulates is staged until the next advance);
 *                                 lsspa_stats_reset zeroes D and s again; lsspa_history_enable(ctx, 0) switches it off
 *   lsspa_error_advance         : fold the staged lift vectors in; they are samples first_id, first_id + stride, ...
 *                                 of the run (the driver deals sample i of a chunk to rank i mod world, so the ids
 *                                 -- hence Xi and every result -- do not depend on the number of ranks)
 *   lsspa_error_running_draws   : x of this context's samples into the draws buffer (lsspa_error_buffer): with
 *                                 several ranks all-reduce it (lsspa_error_allreduce) -- x is linear in (D, s)
 *   lsspa_error_quantiles_enqueue / lsspa_error_result : the quantile kernels, then feature errors, overall error, the
 *                                 running mean and n copied into pinned slot `slot` (0 .. 63) behind an event -- nothing
 *                                 waits.  lsspa_error_result reads a slot: wait != 0 blocks on its event, wait == 0
 *                                 polls (*ready = 0: not yet).  This is what lets the driver evaluate the stop rule of
 *                                 check k while the samples of check k + 1 are already running (they are dropped on a
 *                                 stop), so the estimator is off the critical path.
 *   lsspa_error_state_get / _set: D [1024][p] and s [1024] to / from host memory (checkpoint / resume)
 *   lsspa_error_xi              : test hook -- the normals Xi [1024][count] of `count` sample ids, to host memory */
int lsspa_error_running_enable(lsspa_ctx* ctx, uint64_t seed);
int lsspa_error_advance(lsspa_ctx* ctx, int64_t first_id, int64_t stride);
int lsspa_error_running_draws(lsspa_ctx* ctx, int64_t n_total);
int lsspa_error_quantiles_enqueue(lsspa_ctx* ctx, int32_t slot);
/* one rank: lsspa_error_running_draws + lsspa_error_quantiles_enqueue in one call and two launches -- the quantile
 * kernels evaluate x = (D - s mean^T) / sqrt(n (n - 1)) as they read it, the draws buffer is not written */
int lsspa_error_check_enqueue(lsspa_ctx* ctx, int64_t n_total, int32_t slot);
int lsspa_error_result(lsspa_ctx* ctx, int32_t slot, int32_t wait, int32_t* ready, double* feature_errors,
                       double* overall_error, double* mean, int64_t* n);
/* The per-chunk tail of a launched batch in one call, for hosts whose own call overhead would bound a small problem
 * (a chunk of 256 orderings takes the GPU 37 us at p = 100).  For every chunk c = 0 .. n_chunks - 1, in order:
 * lsspa_lift_collect(ticket, first[c], count[c], NULL, accumulate) -- skipped for count[c] == 0 --; with a communicator
 * of several ranks lsspa_stats_allreduce + lsspa_stats_merge; lsspa_error_advance(first_id[c], stride); and, where
 * n_after[c] > 0, the check of that global sample count into slot[c] (one rank: lsspa_error_check_enqueue; several:
 * lsspa_error_running_draws + lsspa_error_allreduce + lsspa_error_quantiles_enqueue).  Nothing waits; the results are
 * read with lsspa_error_result.  Order and arithmetic are those of the separate calls (ls_spa/ls_spa.py:203-230).
 * One rank, p <= 128, 2 .. 32 chunks of up to 512 samples that follow each other in the batch: the statistics, the
 * estimator's sums and all the checks of the call are five launches (the state after every chunk is kept for the check
 * that belongs to it) -- the numbers are those of the chunk-by-chunk calls to the last bit. */
int lsspa_group_collect(lsspa_ctx* ctx, int32_t ticket, int32_t n_chunks, const int32_t* first, const int32_t* count,
                        const int64_t* first_id, int64_t stride, const int64_t* n_after, const int32_t* slot);
int lsspa_error_state_get(lsspa_ctx* ctx, double* D, double* s);
int lsspa_error_state_set(lsspa_ctx* ctx, const double* D, const double* s);
int lsspa_error_xi(lsspa_ctx* ctx, uint64_t seed, int64_t first_id, int64_t stride, int64_t count, double* xi);

/* (e) -- collectives.  The reference is single-process; these implement the multi-GPU form of its running-statistics
 * merge (ls_spa/ls_spa.py:103-119, :212-216): orderings are dealt over one process per GPU and the ONLY data-path
 * exchange is one SUM all-reduce of the pending-batch moments per chunk.  RCCL over xGMI, resolved
 * at run time (no link-time dependency; a single-GPU process never loads it); every collective is enqueued on the
 * context's stream, so kernels -> all-reduce -> merge run without host synchronisation.
 *   lsspa_comm_unique_id  : 128 opaque bytes made on rank 0 (ncclGetUniqueId) and handed to the other ranks by the
 *                           host (the Python package uses a TCP exchange on MASTER_ADDR); errors: lsspa_last_error(NULL)
 *   lsspa_comm_init       : collective over all ranks; binds the communicator to this context's GPU
 *   lsspa_stats_allreduce : the pending buffer [n_b, S, Q]; from p = 2048 on Q travels as its upper triangle
 *                           (1 + p + p (p + 1) / 2 elements: half the bytes; Q is exactly symmetric)
 *   lsspa_reduce_allreduce: the Gram sums of a row-sharded reduction (between lsspa_reduce_partial and _finish)
 *   lsspa_error_allreduce : the partial draws of the device-side estimator (between lsspa_error_draws and _quantiles)
 *   lsspa_comm_sum_i64    : host integers, summed over the ranks in place (row counts of a sharded reduction)
 *   lsspa_comm_allgather  : host fp64 [count] per rank -> [world][count] (lift vectors for attribution_history) */
#define LSSPA_COMM_ID_BYTES 128
int lsspa_comm_unique_id(uint8_t* id128);
int lsspa_comm_init(lsspa_ctx* ctx, const uint8_t* id128, int32_t rank, int32_t world);
int lsspa_comm_destroy(lsspa_ctx* ctx);
/* rank and size as RCCL reports them for this context's communicator (ncclCommUserRank / ncclCommCount) */
int lsspa_comm_info(const lsspa_ctx* ctx, int32_t* rank, int32_t* world);
int lsspa_stats_allreduce(lsspa_ctx* ctx);
int lsspa_reduce_allreduce(lsspa_ctx* ctx);
int lsspa_error_allreduce(lsspa_ctx* ctx);
int lsspa_comm_sum_i64(lsspa_ctx* ctx, int64_t* values, int32_t count);
int lsspa_comm_allgather(lsspa_ctx* ctx, const double* send, int64_t count, double* recv);

/* per-kernel-class HIP-event timing on the context's stream */
#define LSSPA_K_GATHER 0
#define LSSPA_K_CHOL_DIAG 1
#define LSSPA_K_CHOL_PANEL 2
#define LSSPA_K_STRIP 3
#define LSSPA_K_LIFT 4
#define LSSPA_K_STATS 5
#define LSSPA_K_GRAM 6
#define LSSPA_K_ERROR 7
#define LSSPA_K_COMM 8
#define LSSPA_K_SMALL 9     /* fused small-p kernel: gather .. lifts of one ordering in one workgroup */
#define LSSPA_K_PAIRS 10    /* pair kernels of lsspa_pairs_batch: Delta, per-pair statistics, lift sum */
#define LSSPA_K_COUNT 11
int lsspa_profile_enable(lsspa_ctx* ctx, int32_t on);
int lsspa_profile_get(lsspa_ctx* ctx, int32_t kernel_class, double* total_ms, int64_t* launches);
int lsspa_profile_reset(lsspa_ctx* ctx);

/* developer switches: cross-checks of kernel variants against each other (0 = shipped configuration):
 *   128  tri mode: V by the strip kernel (the shipped path of rect mode) instead of V^T by the panel launches' X tiles
 *   512  tri mode: the lift kernel reads V^T back and scans it, instead of the X tiles scanning their own blocks
 *  1024  general path also for small problems (p + 1 <= 128 normally takes the fused one-workgroup kernel)
 *  4096  fault injection: the L tiles never raise the flag the fused lift scan waits for -- every X tile runs into the
 *        scan's time-out (~0.1 s a launch), LSSPA_INFO_SCAN_WAIT and LSSPA_INFO_SUM are set, nothing hangs
 * 16384  small problems: the LDS-resident kernel also where the register-resident one applies (p + 1 <= 112)
 * 65536  Gram kernel: workgroup id = unit (the units of a row slice spread over the XCDs instead of sharing one L2)
 * Every combination computes the same lifts (tests/test_gpu_kernels.py).  Environment, read once per process:
 * LSSPA_HANDOVER=k moves the point at which the second lane's next launch sequence may start to "after panel launch k"
 * (default: the middle one).  Retired in round 5 (each switched between two code paths that both stay in use and
 * are pinned against the oracle by themselves): 64 plain dispatch order in the panel kernel (what a matrix count that
 * is not a multiple of eight takes), 256 unpaired gather (what antithetical = 0 takes), 2048 no skipping of the
 * all-padding tiles.  Earlier rounds carried more; DESIGN_HISTORY.md. */
int lsspa_set_flags(lsspa_ctx* ctx, int32_t flags);

/* test hooks */
/* the nth device allocation from now on fails with LSSPA_ERR_NOMEM (0 disarms): exercises the out-of-memory
 * paths, after which a context must still be usable (e.g. with a smaller batch) */
int lsspa_debug_fail_alloc(lsspa_ctx* ctx, int32_t nth);
/* use the packed (upper-triangle) form of lsspa_stats_allreduce from this p on (default 2048) */
int lsspa_debug_pack_from(lsspa_ctx* ctx, int32_t p_min);
/* chosen lift vectors in front of the collect paths: lifts [B][p] (host) are copied into the lane's lift buffer and the
 * lane is marked as lsspa_lift_launch leaves it (B samples, none taken), *ticket names it.  lsspa_lift_collect (every
 * accumulate mode), lsspa_lift_collect_chunks, lsspa_group_collect, the history and the running estimator then see
 * those vectors as a batch's; no ordering is factored and no sum is checked.  LSSPA_ERR_STATE with two lanes, with a
 * player map set, with no problem loaded or while a launched batch is uncollected. */
int lsspa_debug_lift_inject(lsspa_ctx* ctx, const double* lifts, int32_t B, int32_t* ticket);
/* how lsspa_lift_collect cuts a chunk of n_samples at dimension p for its moments: *small = 1 if the one-launch forms of
 * small problems take it (p <= 128, up to 512 samples), *n_slices and *per_slice = the slices of the general kernel and
 * the samples each is given (the last ones may get fewer, or none).  No context, no GPU: host code only. */
int lsspa_debug_stats_slices(int32_t n_samples, int32_t p, int32_t* n_slices, int32_t* per_slice, int32_t* small);
/* how a Gram launch of n rows at p features is cut (csrc/k_gram.hip): *n_split = the class-A slice count the library
 * picks for it, cnt3 / slices3 / rps3 = units per slice, row slices and rows per slice of the three unit classes (A:
 * pairs of full tiles, B: pairs with the ragged last tile, C: diagonal duos / a single), *nt = 128-column tiles of
 * [X | y], *xlive = live 16-column blocks of the last tile.  No context, no GPU: host code only. */
int lsspa_debug_gram_plan(int64_t n, int32_t p, int32_t* n_split, int32_t* cnt3, int32_t* slices3, int32_t* rps3,
                          int32_t* nt, int32_t* xlive);
/* what the per-ordering general path launches for n_ord orderings at p features (csrc/k_factor.hip, panel_plan, under
 * the engine's own shape rules: p_pad = p + 1 rounded up to 128, p_live = p + 1 rounded up to 16, two matrices an
 * ordering in tri mode, and in tri mode one more panel launch, X tiles only, unless developer flag 128 is in `flags`):
 * *p_pad, *n_mats, *n_launch panel launches and, for the first `cap` of them, plans [launch][8] = Jo, L tiles per
 * matrix, X tiles per ordering, grouped (the eight-matrices-at-a-time workgroup map), xlast (the instantiation without
 * the last panel's dead columns), workgroups, p_live, orderings as the kernel counts them.  p = 127 in rect mode has
 * no panel launch.  Whether a problem takes the general path at all (p + 1 <= 128 in fp64 tri mode does not, without
 * developer flag 1024) is not this function's business.  No context, no GPU: host code only. */
int lsspa_debug_panel_plan(int32_t p, int32_t n_ord, int32_t tri, int32_t flags, int32_t* p_pad, int32_t* n_mats,
                           int32_t* n_launch, int32_t* plans, int32_t cap);
/* one launch from launch_chol2_panel's own arguments (has_X: X tiles are computed; p_live <= 0 or > p_pad: none
 * known), plan [8] as above; LSSPA_ERR_ARG for what launch_chol2_panel refuses. */
int lsspa_debug_panel_plan_launch(int32_t p_pad, int32_t Jo, int32_t n_mats, int32_t n_ord, int32_t has_X,
                                  int32_t p_live, int32_t* plan);
/* rows per chunk of the streamed reduction of host-resident data, instead of its ~96 MB sizing with a 1024-row floor:
 * 0 (the default sizing again) or a multiple of 16 that is at least 16, anything else is LSSPA_ERR_ARG.  The slice count
 * of every chunk's launch is the one for `rows` rows, as with the default sizing.  Stays set until changed: a
 * reduction does not reset it.  A test reaches three and more chunks, a short last one and the accumulating forms of
 * both reduce kernels with a small matrix through it. */
int lsspa_debug_reduce_chunk_rows(lsspa_ctx* ctx, int64_t rows);
/* Host helper of the QMC ordering sources (the reference: np.argsort of Sobol' points / projected normals,
 * experiments/ground_truth_medium.py:56-71): out [B][p] = the argsort of every row of keys [B][p], on up to `threads`
 * threads of this library (no interpreter lock between them and the caller's other threads).  A row with all keys
 * different has one argsort; redo[s] = 1 marks the rows with equal keys or a NaN, whose order is numpy's own business:
 * the caller sorts those with numpy (*n_redo of them).  No context, no GPU. */
int lsspa_host_argsort_rows(const double* keys, int64_t B, int32_t p, int32_t* out, uint8_t* redo, int32_t threads,
                            int64_t* n_redo);
/* The 'argsort' ordering source as a thread of this library (the reference: np.argsort(qmc.Sobol(p, seed).random(n), axis=1),
 * experiments/ground_truth_medium.py:56-60): Sobol' points by SciPy's own recurrence -- the caller reads direction numbers
 * sv [p][bits], the state before the first step q0 [p] and the scale off a SciPy engine it built, having checked them
 * against that engine's output -- and their row argsort, drawn `block` orderings at a time up to `ahead` ahead of the
 * consumer (`ahead_unasked` until the first lsspa_sampler_take) on `threads` sort threads; ordering number g of the run
 * belongs to rank g mod world, only those rows are sorted and handed out.  lsspa_sampler_take: the next `count`
 * orderings of the run -- *n_taken of them exist --, this rank's rows of them into out [cap][p] (*n_own rows); rows with
 * equal keys (numpy's order among them is its own) are listed by position in `out` and number in the run: the caller
 * sorts those with numpy.  Errors of these three calls are read with lsspa_last_error(NULL).  No context, no GPU. */
int lsspa_sampler_create(int32_t p, int32_t bits, const uint64_t* sv, const uint64_t* q0, double scale, int64_t limit,
                         int32_t block, int64_t ahead, int64_t ahead_unasked, int32_t threads, int32_t rank,
                         int32_t world, void** out);
int lsspa_sampler_take(void* sampler, int64_t count, int32_t* out, int64_t cap, int64_t* n_taken, int64_t* n_own,
                       int64_t* redo_pos, int64_t* redo_id, int64_t* n_redo);
int lsspa_sampler_destroy(void* sampler);
/* overwrite the R^2 the batches' sums are checked against (LSSPA_INFO_SUM; set by lsspa_full_fit): a test makes the
 * check fire on a healthy engine with it */
int lsspa_debug_set_r2(lsspa_ctx* ctx, double r2);
/* 1 if every row of perms [B][p] is a permutation of 0..p-1, else 0 -- the check every batch launch makes on the host
 * (csrc/host_perms.cpp: 128-bit sets by AVX2 for 8 <= p <= 128, a stamp array otherwise); plain != 0: the stamp loop
 * alone.  No context, no GPU: host code only. */
int lsspa_debug_check_perms(const int32_t* perms, int32_t B, int32_t p, int32_t plain);
int lsspa_mfma_probe(lsspa_ctx* ctx, const double* A16x4, const double* B4x16, double* D16x16, int32_t dtype);
/* factor one ordering and copy the padded factor(s) out: L [p_pad][p_pad] (train),
 * Lt [p_pad][p_pad] (test, tri mode only, else untouched), V [n_iblk*64][m_pad] */
int lsspa_debug_factor(lsspa_ctx* ctx, const int32_t* perm, double* L, double* Lt, double* V,
                       int32_t* p_pad, int32_t* m_pad, int32_t* v_rows);

#ifdef __cplusplus
}
#endif
#endif /* LSSPA_H */
