// C ABI of the LS-SPA engine (include/lsspa.h): context, device memory and the
// orchestration of the per-batch kernel sequence
//     gather -> { chol_diag, chol_panel } x nblk -> strip -> lift -> stats
#include "../../include/lsspa.h"

#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "comm.h"
#include "kernels.h"
#include "tiles.h"

using namespace lsspa;

namespace {

thread_local std::string g_create_error;

struct ProfRec {
  int cls;
  hipEvent_t beg, end;
};

template <typename T>
struct DevBuf {
  T* ptr = nullptr;
  size_t count = 0;
};

template <typename T>
void dev_free(DevBuf<T>& b) {
  if (b.ptr) (void)hipFree(b.ptr);
  b.ptr = nullptr;
  b.count = 0;
}

// What an exact enumeration keeps between calls (lsspa_subsets_shapley, lsspa_groups_shapley): its own buffers and info
// word, nothing of the sampling path's, and the timing of its last call.  The context holds one per entry point.
struct ExactWork {
  DevBuf<double> Hh, w, part, out, vals;   // rect-mode test Gram, Shapley weights, partial table, its sums, debug values
  DevBuf<uint64_t> masks;                  // the debug values' subsets
  DevBuf<int32_t> info, tab;               // info word; GroupLayout::tab (groups only)
  DevBuf<uint32_t> best;                   // the selection calls' masks beside part's values (best_run, top_run)
  double kernel_ms = 0.0, max_launch_ms = 0.0;
  int64_t launches = 0;
  void release() {
    dev_free(Hh); dev_free(w); dev_free(part); dev_free(out); dev_free(vals);
    dev_free(masks); dev_free(info); dev_free(tab); dev_free(best);
  }
};

// What the bootstrap keeps (lsspa_boot_load .. lsspa_boot_free): the rows of both sides and the buffers of one block of
// replicates.  Nothing of the loaded problem, the sampling path or the exact enumerations' state is in here, and a
// reduction does not touch it.
struct BootWork {
  bool loaded = false;
  int p = 0;
  int64_t n[2] = {0, 0};                   // rows: train, test
  double reg = 0.0;
  DevBuf<double> Z0, Z1;                   // [n][ldz] rows [X | y] of the two sides, zero-padded columns
  DevBuf<char> stage_x, stage_y;           // host rows on their way into Z
  DevBuf<uint32_t> cnt0, cnt1;             // [block][n] bootstrap counts
  DevBuf<double> wt0, wt1;                 // [block][n] caller's weights
  DevBuf<double> part0, part1, S0, S1, wsum;   // Gram partials, their sums [block][c][c], sum of the training weights
  DevBuf<double> G, g, H, h, inv_yy;       // the block's reduced problems
  DevBuf<double> w, epart, eout;           // Shapley weights, the enumeration's partial table and its column sums
  DevBuf<int32_t> info;                    // [block]
  DevBuf<int32_t> tab;                     // GroupLayout::tab (lsspa_boot_groups_run)
  DevBuf<uint32_t> ebest;                  // lsspa_boot_best_run: (mask, found) beside epart's values, one launch's replicates
  double ms[3] = {0.0, 0.0, 0.0};          // kernel ms of the last run: counts, Gram (to the reduced problems), enumeration
  DevBuf<double>& Z(int s) { return s ? Z1 : Z0; }
  DevBuf<uint32_t>& cnt(int s) { return s ? cnt1 : cnt0; }
  DevBuf<double>& wt(int s) { return s ? wt1 : wt0; }
  DevBuf<double>& part(int s) { return s ? part1 : part0; }
  DevBuf<double>& S(int s) { return s ? S1 : S0; }
  void release() {
    dev_free(Z0); dev_free(Z1); dev_free(stage_x); dev_free(stage_y); dev_free(cnt0); dev_free(cnt1);
    dev_free(wt0); dev_free(wt1); dev_free(part0); dev_free(part1); dev_free(S0); dev_free(S1); dev_free(wsum);
    dev_free(G); dev_free(g); dev_free(H); dev_free(h); dev_free(inv_yy); dev_free(w); dev_free(epart);
    dev_free(eout); dev_free(info); dev_free(tab); dev_free(ebest);
    loaded = false;
  }
};

// What the K-fold cross-validation keeps (lsspa_cv_load .. lsspa_cv_free): the packed rows, the K fold problems in the
// replicate layout the enumerations read (device; G, g, H, h and the pooled 1 / ||y||^2 also on the host as they were
// computed), the enumerations' tables and the last calls' timing.  Nothing of the loaded problem, the sampling path, the
// exact enumerations' or the bootstrap's state is in here.
struct CvWork {
  bool loaded = false;
  int p = 0, K = 0;
  int64_t n = 0;
  DevBuf<double> Z;                        // [n][ldz] rows [X | y]
  DevBuf<char> stage_x, stage_y;           // host rows on their way into Z
  DevBuf<int32_t> fid, nf;                 // [n] fold labels, [K] fold sizes
  DevBuf<double> wt, gpart, S;             // [K][n] indicator weights, Gram partials, S_f [K][c][c]
  DevBuf<double> G, g, H, h, inv_yy;       // the fold problems [K]...
  std::vector<double> Gh, gh, Hh, hh, yh;  // the same on the host
  DevBuf<double> w, part, out, phi, vals;  // Shapley weights, partial table, its sums, phi_fold | phi, debug values
  DevBuf<double> gw;                       // the grouped calls' Shapley weights (of g players; w is of p, p <= 32 only)
  DevBuf<int32_t> tab;                     // and their layout table (GroupLayout::tab)
  DevBuf<uint64_t> masks;
  DevBuf<int32_t> info, dinfo;             // [K] info words of a call; the debug values' own
  DevBuf<uint32_t> best;                   // the selection calls' masks beside part's values (best_run, top_run)
  double gram_ms = 0.0, enum_ms = 0.0, max_launch_ms = 0.0;
  int64_t launches = 0;
  // The ridge path's own (lsspa_cv_path_shapley, lsspa_cv_path_groups_shapley): the problems of a block of ridge values
  // [Lb K]..., written from S, and everything its launches write.  Of the above it reads S, nf, w (gw, tab: uploaded by
  // every grouped call) and writes the timing.
  struct Path {
    DevBuf<double> regs, G, g, H, h, inv_yy; // [Lb] ridge values; the problems (l, f), l-major
    DevBuf<double> part, out, phi, vals;     // partial table, its sums [Lb K][cols], phi_fold | phi, the full masks' values
    DevBuf<uint64_t> masks;
    DevBuf<int32_t> info, dinfo;             // [Lb K] info words of the enumeration; the values' own
    void release() {
      dev_free(regs); dev_free(G); dev_free(g); dev_free(H); dev_free(h); dev_free(inv_yy); dev_free(part);
      dev_free(out); dev_free(phi); dev_free(vals); dev_free(masks); dev_free(info); dev_free(dinfo);
    }
  } path;
  void release() {
    dev_free(Z); dev_free(stage_x); dev_free(stage_y); dev_free(fid); dev_free(nf); dev_free(wt); dev_free(gpart);
    dev_free(S); dev_free(G); dev_free(g); dev_free(H); dev_free(h); dev_free(inv_yy); dev_free(w); dev_free(part);
    dev_free(out); dev_free(phi); dev_free(vals); dev_free(masks); dev_free(info); dev_free(dinfo); dev_free(best);
    dev_free(gw); dev_free(tab);
    path.release();
    loaded = false;
  }
};

// The reduced form of m responses on one design: the shared G and H, one g and h per response and the test responses'
// squared norms, on the host as they were stored (the *_get_gram entry points) and G, H, g, h on the device.  A member of
// MultiWork and MultiLiftWork; the permutation test reaches it through its MultiWork.  reduced_store fills it.
struct ReducedForm {
  int p = 0, m = 0;
  std::vector<double> Gh, Hh, gh, hh, yyh; // [p][p], [p][p], [m][p], [m][p], [m]
  DevBuf<double> G, H, g, h;               // the first four on the device
  void release() { dev_free(G); dev_free(H); dev_free(g); dev_free(h); }
};

// What the multi-response enumeration keeps (lsspa_multi_load / lsspa_multi_set_reduced .. lsspa_multi_free): the shared
// G and H, one g, h and 1 / ||y||^2 per response, the buffers of one block of responses and the last call's timing.
// Nothing of the loaded problem, the sampling path, the exact enumerations' or the bootstrap's state is in here.
struct MultiWork {
  bool loaded = false;
  ReducedForm rf;
  DevBuf<double> inv_yy;                   // [m]
  DevBuf<double> w, part, out, vals;       // Shapley weights, partial table of a block, its column sums, debug values
  DevBuf<uint64_t> masks;
  DevBuf<int32_t> info, tab;               // tab: the layout of the last grouped call (GroupLayout::tab)
  double gram_ms = 0.0, enum_ms = 0.0, max_launch_ms = 0.0;
  int64_t launches = 0;
  void release() {
    rf.release(); dev_free(inv_yy); dev_free(w); dev_free(part); dev_free(out); dev_free(vals);
    dev_free(masks); dev_free(info); dev_free(tab);
    loaded = false;
  }
};

// What the three sampled families (lsspa_multi_lift_*, lsspa_cv_lift_*, lsspa_boot_lift_*) each keep one of ------------
// A family's own player map (lift_players_set; not ctx->players): ng != 0 makes a sample g group lifts, and the
// orderings given are orderings of the groups, expanded on the host as they are staged (lift_stage_rows).
struct LiftPlayers {
  int ng = 0;                              // groups of the player map (0: none)
  PlayerMap map;
  DevBuf<int32_t> pl_off, pl_cols;         // the map's CSR on the device
  std::vector<int32_t> rows;               // a launch's expanded rows on the host
  int sd(int p) const { return ng ? ng : p; }                   // the dimension of a sample
  int64_t rows_per(int per) const { return ng ? per : 1; }      // rows of perms a sample takes on the device
  const int32_t* off() const { return ng ? pl_off.ptr : nullptr; }
  const int32_t* cols() const { return ng ? pl_cols.ptr : nullptr; }
  void release() {
    dev_free(pl_off); dev_free(pl_cols);
    ng = 0;
  }
};

// The running (n, mean, M2) of a family's samples, `entries` doubles each (lift_stats_*).
struct LiftStats {
  int64_t n = 0;                           // samples folded into (mean, M2)
  DevBuf<double> mean, M2;
  void release() {
    dev_free(mean); dev_free(M2);
    n = 0;
  }
};

// Problems kept at the ordering kernels' stride: G, H [count][LD][LD] and g, h [count][LD] in rows of LD = CV_LIFT_LD
// doubles, the pooled 1 / ||y||^2 [count] and the augmented rows' diagonals [count][2] (lift_problems_*).
struct LiftProblems {
  static constexpr int64_t LD = CV_LIFT_LD, LL = LD * LD;
  DevBuf<double> G, g, H, h, inv_yy, aug;
  void release() { dev_free(G); dev_free(g); dev_free(H); dev_free(h); dev_free(inv_yy); dev_free(aug); }
};
static_assert(BOOT_LIFT_LD == CV_LIFT_LD && BOOT_LIFT_MAX_P == CV_LIFT_MAX_P,
              "the sampled bootstrap keeps its problems at the fold launch's stride");

// What the sampled attribution of many responses keeps (lsspa_multi_lift_load / lsspa_multi_lift_set_reduced ..
// lsspa_multi_lift_free): the reduced form, the orderings and lift vectors [samples][m][d] of one launch, the running
// statistics [m][d] and the last calls' timing.  Nothing of the loaded problem, the sampling path's statistics, the
// enumerations, the bootstrap or lsspa_multi_* is in here.
struct MultiLiftWork {
  bool loaded = false;
  ReducedForm rf;
  LiftPlayers pl;
  LiftStats st;                            // [m][p] allocated, the first m d entries used
  int sd() const { return pl.sd(rf.p); }
  double aug[2] = {1.0, 1.0};              // diagonal of the augmented rows (MultiLiftArgs::aug)
  DevBuf<double> yy;                       // [m]
  DevBuf<double> lifts;                    // [samples of a launch][m][d]
  DevBuf<int32_t> perms, info;             // [samples of a launch][p]; the info word
  double gram_ms = 0.0, batch_ms = 0.0, stats_ms = 0.0;
  void release() {
    rf.release(); pl.release(); st.release(); dev_free(yy); dev_free(lifts); dev_free(perms); dev_free(info);
    loaded = false;
  }
};

// What the sampled K-fold CV attribution keeps (lsspa_cv_lift_load .. lsspa_cv_lift_free): the K fold problems (dense
// on the host too), the orderings, raw lifts and samples of one launch, the running statistics [K + 1][d] and the last
// calls' timing.  Nothing of the loaded problem, lsspa_cv_*, lsspa_multi_lift_* or any other store is in here.
struct CvLiftWork {
  bool loaded = false;
  int p = 0, K = 0;
  LiftPlayers pl;
  LiftStats st;                            // [K + 1][p] allocated, the first (K + 1) d entries used
  LiftProblems pr;                         // [K] (inv_yy, aug: CV_MAX_FOLDS)
  int sd() const { return pl.sd(p); }
  std::vector<double> Gh, gh, Hh, hh, yh;  // [K][p][p], [K][p], .., [K] on the host
  DevBuf<double> raw, batch;               // [orderings of a launch][K][p]; [samples of a launch][K + 1][d]
  DevBuf<int32_t> perms, info;             // a launch's rows; [K] info words
  double gram_ms = 0.0, batch_ms = 0.0, stats_ms = 0.0;
  void release() {
    pl.release(); st.release(); pr.release(); dev_free(raw); dev_free(batch); dev_free(perms); dev_free(info);
    loaded = false;
  }
};

// What the bootstrap of the sampled attribution keeps (lsspa_boot_lift_load .. lsspa_boot_lift_free): the rows of both
// sides, the one set of orderings every replicate shares, and the buffers of one block of replicates -- weights, Gram
// partials and sums, the block's problems, one launch's raw lifts, the replicates' running (mean, M2) [block][d].
// Nothing of the loaded problem, lsspa_boot_*, lsspa_cv_lift_*, lsspa_multi_lift_* or any other store is in here.
struct BootLiftWork {
  bool loaded = false;
  int p = 0;
  int64_t n[2] = {0, 0};                   // rows: train, test
  double reg = 0.0;
  LiftPlayers pl;
  LiftProblems pr;                         // [block]
  int sd() const { return pl.sd(p); }
  int64_t n_samples = 0;                   // samples of the orderings set (0: none)
  int per = 1;                             // orderings a sample (2: antithetical)
  DevBuf<int32_t> perms;                   // the orderings' rows, expanded
  DevBuf<double> Z0, Z1;                   // [n][ldz] rows [X | y] of the two sides, zero-padded columns
  DevBuf<char> stage_x, stage_y;
  DevBuf<uint32_t> cnt0, cnt1;             // [block][n] bootstrap counts
  DevBuf<double> wt0, wt1;                 // [block][n] caller's weights
  DevBuf<double> part0, part1, S0, S1, wsum;
  DevBuf<double> raw, mean, M2, samples;   // one launch's raw lifts; [block][d] twice; one launch's samples (test hook)
  DevBuf<int32_t> info;                    // [block]
  double ms[4] = {0.0, 0.0, 0.0, 0.0};     // kernel ms of the last pass: counts, Gram (to the problems), lifts, statistics
  int64_t launches = 0;                    // its lift launches
  DevBuf<double>& Z(int s) { return s ? Z1 : Z0; }
  DevBuf<uint32_t>& cnt(int s) { return s ? cnt1 : cnt0; }
  DevBuf<double>& wt(int s) { return s ? wt1 : wt0; }
  DevBuf<double>& part(int s) { return s ? part1 : part0; }
  DevBuf<double>& S(int s) { return s ? S1 : S0; }
  void release() {
    dev_free(Z0); dev_free(Z1); dev_free(stage_x); dev_free(stage_y); dev_free(cnt0); dev_free(cnt1);
    dev_free(wt0); dev_free(wt1); dev_free(part0); dev_free(part1); dev_free(S0); dev_free(S1); dev_free(wsum);
    pl.release(); pr.release(); dev_free(raw); dev_free(mean); dev_free(M2); dev_free(samples); dev_free(info);
    dev_free(perms);
    loaded = false;
    n_samples = 0;
  }
};

// What the permutation test keeps (lsspa_perm_load .. lsspa_perm_free): X and y of both sides on the device, the shared
// G and H and the observed g, h, the index rows of two blocks of replicates (device and pinned host: the next block is
// drawn and uploaded while this one runs), the partials of one block, and a MultiWork of its own whose response slots
// the reduce kernel writes and the enumerations of lsspa_multi_* read.  Nothing of the loaded problem, the sampling path,
// the exact enumerations, the bootstrap, lsspa_multi_* or lsspa_multi_lift_* is in here.
struct PermWork {
  bool loaded = false;
  int p = 0;
  int64_t n[2] = {0, 0};                   // rows: train, test
  DevBuf<double> X0, X1, y0, y1;           // [n][ldx] zero-padded columns; [n]
  DevBuf<char> stage_x, stage_y;           // host rows on their way in
  DevBuf<uint32_t> idx[2][2];              // [buffer][side]: [block][ldi]
  uint32_t* pin[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // the same in pinned host memory
  size_t pin_count[2][2] = {{0, 0}, {0, 0}};
  DevBuf<double> part0, part1;             // [slices][ceil(block / 16)][cb][256]
  DevBuf<double> obs_g, obs_h;             // [p] the observed g, h on the device
  MultiWork mw;                            // the reduced form (m = 1); g, h, inv_yy of one block of replicates
  double ms[4] = {0.0, 0.0, 0.0, 0.0};     // last run: draw (host), upload (host), X^T y kernels, enumeration
  DevBuf<double>& X(int s) { return s ? X1 : X0; }
  DevBuf<double>& y(int s) { return s ? y1 : y0; }
  DevBuf<double>& part(int s) { return s ? part1 : part0; }
  void release() {
    dev_free(X0); dev_free(X1); dev_free(y0); dev_free(y1); dev_free(stage_x); dev_free(stage_y);
    dev_free(part0); dev_free(part1); dev_free(obs_g); dev_free(obs_h);
    for (int b = 0; b < 2; ++b)
      for (int s = 0; s < 2; ++s) {
        dev_free(idx[b][s]);
        if (pin[b][s]) (void)hipHostFree(pin[b][s]);
        pin[b][s] = nullptr;
        pin_count[b][s] = 0;
      }
    mw.release();
    loaded = false;
  }
};

}  // namespace

// One lane = everything a batch of orderings needs while its kernels run: work matrices, solve results, staged
// orderings, its lift vectors.  With one lane (default) every batch runs on the context's stream, one after the
// other.  With two lanes (lsspa_set_lanes) successive batches alternate between two workspaces on two streams: the
// kernels of batch k+1 are in flight while batch k drains its launch tails, runs its memory-bound stages or waits
// for its collective -- the statistics (pending buffer, all-reduce, merge) stay in batch order on the context's
// stream.  A lane's batch starts when the other lane's batch is about half done (ev_mid), so the two are in
// different stages (gather / early panels of one beside the late panels / strip of the other) instead of in step.
struct Lane {
  hipStream_t st = nullptr;          // own stream (two-lane mode)
  int cap_ord = 0;                   // orderings the workspace can hold
  int cap_samples = 0;               // samples the lifts buffer can hold
  DevBuf<char> A, V, Dinv;           // raw bytes: esz() per element
  DevBuf<double> Ppart, lifts, diag0;
  DevBuf<double> folded;             // player map set: [samples][g] group lifts, what collect reads instead of lifts
  DevBuf<double> run;                // [cap_ord][p_pad] running sums of the fused lift scan (tri mode)
  DevBuf<int32_t> row_flags;         // [2 cap_ord] "row p of panel J is final" per work matrix (fused lift scan)
  DevBuf<int32_t> perms_d;
  // pinned staging of the orderings: two buffers in turn, each guarded by the event of its last
  // H2D copy, so the host can prepare batch k+1 while the GPU still runs batch k (no stream sync)
  int32_t* perms_h[2] = {nullptr, nullptr};
  hipEvent_t perms_ev[2] = {nullptr, nullptr};
  bool perms_busy[2] = {false, false};
  int perms_turn = 0;
  size_t perms_h_count = 0;
  // the device side is double-buffered too ([2][cap_ord][p]) and fed by a copy stream, so the H2D copy of
  // batch k+1 runs under the kernels of batch k instead of between two batches on the compute stream
  hipStream_t copy_stream = nullptr;
  hipEvent_t perms_used[2] = {nullptr, nullptr};   // the kernels that read device slot b have run
  bool perms_used_valid[2] = {false, false};
  const int32_t* perms_cur = nullptr;              // device slot of the batch being launched
  bool sum_checked = false;                        // the batch's kernel checked the orderings' sums itself
  bool perms_fwd_only = false;                     // ... which holds the samples' orderings only, not their reverses
  // second stream for the two-slice schedule of a batch (developer flag 32)
  // two-lane hand-offs
  hipEvent_t ev_mid = nullptr, ev_done = nullptr, ev_consumed = nullptr, ev_main = nullptr;
  bool mid_valid = false, done_valid = false, consumed_valid = false;
  bool mid_armed = false;            // the batch being launched still has to record ev_mid
  int64_t problem_seen = -1;         // ctx->problem_epoch this lane's stream has been ordered behind
  int B = 0, per = 1, taken = 0;     // the batch in flight (launched, `taken` of its B samples collected so far)
  bool in_flight = false;
};

struct lsspa_ctx {
  int device = 0;
  int n_cu = 256;                // compute units of the device (hipDeviceProp_t::multiProcessorCount)
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;

  // reduced problem
  bool have_problem = false;
  int p = 0, p_pad = 0, m = 0, m_pad = 0, tri = 0;
  double aug_train = 0.0, y_norm_sq = 0.0;
  double r2 = 0.0;               // R^2 of the full model (lsspa_full_fit): what every lift vector must sum to
  bool r2_valid = false;
  bool r2_f32 = false;           // ... computed while the per-ordering work was fp32 (good to 1e-4, not 1e-9)
  double min_rel_pivot = 1.0;    // smallest L_jj^2 / G_jj (tri: and H_jj) of the identity ordering's factors (lsspa_full_fit)
  DevBuf<double> G, g, H, h, Ft, ytil, scal;
  DevBuf<float> Gf, Hf;        // fp32 copies of G / H for the fp32 gather, made on first use
  bool src_f32_valid = false;

  // per-batch workspace: one or two LANES (struct Lane above), used in turn by successive batches
  int f32 = 0;          // element type of the per-ordering work matrices (0: double, 1: float)
  size_t esz() const { return f32 ? 4 : 8; }
  DevBuf<int32_t> info_d;
  Lane lanes[2];
  int n_lanes = 1;      // lsspa_set_lanes
  int lane_turn = 0;    // lane of the next batch
  int lane_last = 0;    // lane of the most recent batch (its lifts are what lsspa_full_fit etc. read)
  hipStream_t lane_stream(const Lane& L) const { return n_lanes == 1 ? stream : L.st; }
  // two lanes: what the lanes' streams must see of the context's stream -- the loaded problem and its fp32 copies.
  // An event recorded there whenever those change (problem_epoch counts the changes).
  hipEvent_t ev_problem = nullptr;
  int64_t problem_epoch = 0;

  // running statistics
  DevBuf<double> mean, M2, pend, state_n, stat_parts;
  DevBuf<double> mean_alt, state_alt;   // the other halves of the (mean, n) pair: lsspa_lift_collect(accumulate = 2)
  bool pend_dirty = false;
  // history of lift vectors + device-side error estimator
  DevBuf<double> hist, xi_d, draws, err_out;
  // row-sharded reduction in progress: summed Gram buffers [2][P1pad][P1pad]
  DevBuf<double> Cred;
  bool reduce_open = false;
  int64_t hist_cap = 0, hist_n = 0;
  // player map (lsspa_set_players): groups of columns are the players; g_players = 0: none, the columns are
  PlayerMap players;
  int g_players = 0;
  DevBuf<int32_t> pl_off, pl_cols;   // the map's CSR on the device
  // sampled pairwise interactions (lsspa_pairs_*): per-pair tables [d][d] kept at [a][b], a < b; the sum of all lift
  // vectors; per-batch Delta / inverse orderings / orderings; injected lifts (test hook).  pairs_d = sd() when enabled.
  bool pairs_on = false;
  int pairs_d = 0;
  int64_t pairs_n = 0;
  DevBuf<int64_t> pr_count;
  DevBuf<double> pr_mean, pr_m2, pr_phi, pr_delta, pr_lifts;
  DevBuf<int16_t> pr_pos;
  DevBuf<int32_t> pr_perms;
  int32_t* pr_perms_h = nullptr;     // pinned staging of a batch's orderings, guarded by the event of its upload
  size_t pr_perms_h_count = 0;
  hipEvent_t pr_ev = nullptr;
  bool pr_ev_busy = false;
  std::vector<int32_t> pr_rows;      // the 3 B expanded rows of a batch
  // dimension of a SAMPLE -- lift vector handed to collect, running statistics, history, estimator, results.  The
  // factorisation side (orderings the kernels see, work matrices, the un-folded lift buffer) keeps p.
  int sd() const { return g_players ? g_players : p; }
  int ldh() const { return ((sd() + 127) / 128) * 128; }
  // running form of the estimator (lsspa_error_running_*): D = Xi L, s = Xi 1 of the samples folded in so far; the
  // history buffer then only stages the lift vectors between a collect and the next lsspa_error_advance
  bool run_on = false;
  uint64_t run_seed = 0;
  DevBuf<double> Dacc, sacc;
  static constexpr int RES_SLOTS = 64;
  double* res_h = nullptr;            // pinned [RES_SLOTS][2 p + 2]: feature errors, overall error, mean, n
  double* res_hd = nullptr;           // the same memory as the device sees it: the quantile kernel writes a check's
                                      // results there itself (no copy in the chain of a check)
  size_t res_h_count = 0;
  hipEvent_t res_ev[RES_SLOTS] = {nullptr};
  bool res_valid[RES_SLOTS] = {false};
  int res_via[RES_SLOTS] = {0};       // the slot whose event covers this one (itself, or the last check of its group)
  int flags = 0;
  // collectives (RCCL), see comm.h
  Comm* comm = nullptr;
  DevBuf<double> pack, xfer;     // packed moments; staging of host-side all-gathers
  DevBuf<double> theta_d;        // lsspa_full_fit's back-substitution
  // exact attribution by subset enumeration (lsspa_subsets_shapley) and over groups of columns (lsspa_groups_shapley)
  ExactWork sub, grp;
  BootWork boot;                 // bootstrap of the exact attribution (lsspa_boot_*)
  CvWork cv;                     // K-fold cross-validation (lsspa_cv_*)
  MultiWork multi;               // exact attribution of many responses at once (lsspa_multi_*)
  MultiLiftWork mlift;           // sampled attribution of many responses (lsspa_multi_lift_*)
  CvLiftWork cvlift;             // sampled attribution of the K-fold cross-validated R^2 (lsspa_cv_lift_*)
  BootLiftWork bootlift;         // bootstrap of the sampled attribution (lsspa_boot_lift_*)
  PermWork perm;                 // permutation test of the exact attribution (lsspa_perm_*)
  DevBuf<double> mean_snap, n_snap;   // running mean / n after every chunk of a group folded in one launch (small p)
  DevBuf<double> grp_P, grp_S, grp_D, grp_s, grp_norms;   // launch_error_group: products, sums and their snapshots
  // the streamed reduction's staging (two row chunks in flight), its copy stream and events: kept between calls
  DevBuf<char> red_x[2], red_y[2];
  hipStream_t red_cs = nullptr;
  hipEvent_t red_copied[2] = {nullptr, nullptr}, red_consumed[2] = {nullptr, nullptr};
  DevBuf<int64_t> ibuf;
  int pack_from_p = 2048;        // the moments travel as an upper triangle from this p on
  std::vector<int32_t> perm_mark;   // scratch of the ordering validation
  bool general_path_once = false;   // set while the factors themselves are wanted (full_fit, get_factors, debug_factor)
  int fail_alloc_in = 0;   // test hook (lsspa_debug_fail_alloc): the n-th device allocation from now fails
  int64_t red_chunk_rows = 0;   // test hook (lsspa_debug_reduce_chunk_rows): rows per streamed chunk, 0 = default sizing

  // host seconds of the last reduction's parts (lsspa_reduce_timing): streamed copies + Gram kernels, finalize
  // (scaling, Cholesky-side set-up of the statistics, sync)
  double red_stream_s = 0.0, red_finalize_s = 0.0;

  // profiling
  bool prof_on = false;
  std::vector<ProfRec> prof_recs;
  double prof_ms[LSSPA_K_COUNT] = {0};
  int64_t prof_n[LSSPA_K_COUNT] = {0};

  int fail(int code, const char* what, hipError_t e = hipSuccess) {
    char buf[512];
    if (e != hipSuccess)
      snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else
      snprintf(buf, sizeof buf, "%s", what);
    err = buf;
    return code;
  }
};

namespace {

#define HIPCHK(expr)                                              \
  do {                                                            \
    hipError_t e_ = (expr);                                       \
    if (e_ != hipSuccess) return ctx->fail(LSSPA_ERR_HIP, #expr, e_); \
  } while (0)

template <typename T>
int dev_alloc(lsspa_ctx* ctx, DevBuf<T>& b, size_t count) {
  if (b.count >= count && b.ptr) return LSSPA_OK;
  if (b.ptr) (void)hipFree(b.ptr);
  b.ptr = nullptr;
  b.count = 0;
  if (ctx->fail_alloc_in > 0 && --ctx->fail_alloc_in == 0)
    return ctx->fail(LSSPA_ERR_NOMEM, "hipMalloc: out of memory (injected by lsspa_debug_fail_alloc)");
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&b.ptr), count * sizeof(T));
  if (e != hipSuccess) {
    b.ptr = nullptr;
    (void)hipGetLastError();
    return ctx->fail(LSSPA_ERR_NOMEM, "hipMalloc", e);
  }
  b.count = count;
  return LSSPA_OK;
}

#define TRY(expr)                     \
  do {                                \
    int rc_ = (expr);                 \
    if (rc_ != LSSPA_OK) return rc_;  \
  } while (0)

// A player map from labels (NULL: no map) into map / off / cols / ng, for lsspa_set_players and the sampled families'
// own maps: the refusals (null_msg: the entry point's, for NULL labels with g != 0), then quiesce() -- the caller's wait
// for work that may still read the tables, and whatever it resets with it -- then the allocations and the upload.
template <typename Quiesce>
int player_map_set(lsspa_ctx* ctx, const char* null_msg, const int32_t* labels, int p, int g, Quiesce&& quiesce,
                   PlayerMap& map, DevBuf<int32_t>& off, DevBuf<int32_t>& cols, int& ng) {
  if (!labels && g != 0) return ctx->fail(LSSPA_ERR_ARG, null_msg);
  PlayerMap built;
  if (labels)
    if (const char* why = player_map_build(labels, p, g, built)) return ctx->fail(LSSPA_ERR_ARG, why);
  TRY(quiesce());
  if (!labels) {
    ng = 0;
    return LSSPA_OK;
  }
  TRY(dev_alloc(ctx, off, (size_t)p + 1));
  TRY(dev_alloc(ctx, cols, (size_t)p));
  HIPCHK(hipMemcpy(off.ptr, built.off.data(), sizeof(int32_t) * built.off.size(), hipMemcpyHostToDevice));
  if (!built.cols.empty())     // (every column in the baseline cannot be: g >= 1 groups own one each; kept as a guard)
    HIPCHK(hipMemcpy(cols.ptr, built.cols.data(), sizeof(int32_t) * built.cols.size(), hipMemcpyHostToDevice));
  map = std::move(built);
  ng = g;
  return LSSPA_OK;
}

inline int round_up(int x, int q) { return ((x + q - 1) / q) * q; }

// The shape rules of the general path, in one place for set_dims, run_slice and lsspa_debug_panel_plan:
// the two-level factorisation walks 128-wide panels of the p features and the carried row;
inline int work_p_pad(int p) { return round_up(p + 1, 128); }
// rows and columns of a work matrix at or beyond this are identity / zero padding, written by the gather;
inline int work_p_live(int p) { return round_up(p + 1, 16); }
// tri mode computes V^T inside the panel launches; rect mode (and developer flag 128) uses the strip kernel;
inline bool vt_rule(int tri, int flags) { return tri && !(flags & 128); }
// panel steps Jo = 0 .. p_pad / 128 - 2; with V^T one more (X tiles only): step Jo also computes block column Jo of V^T
inline int panel_launches(int p_pad, bool vt) { return p_pad / 128 - 1 + (vt ? 1 : 0); }

struct ProfScope {
  lsspa_ctx* ctx;
  ProfRec rec;
  bool live;
  hipStream_t st;
  ProfScope(lsspa_ctx* c, int cls, hipStream_t on = nullptr) : ctx(c), live(false), st(on) {
    if (!c || !c->prof_on) return;
    if (!st) st = c->stream;
    rec.cls = cls;
    if (hipEventCreate(&rec.beg) != hipSuccess) return;
    if (hipEventCreate(&rec.end) != hipSuccess) {
      (void)hipEventDestroy(rec.beg);
      return;
    }
    (void)hipEventRecord(rec.beg, st);
    live = true;
  }
  ~ProfScope() {
    if (!live) return;
    (void)hipEventRecord(rec.end, st);
    try {
      ctx->prof_recs.push_back(rec);
    } catch (...) {   // out of host memory: lose the sample, not the process (a throwing destructor terminates)
      (void)hipEventDestroy(rec.beg);
      (void)hipEventDestroy(rec.end);
    }
  }
};

int sync_all(lsspa_ctx* ctx);

int prof_collect(lsspa_ctx* ctx) {
  if (ctx->prof_recs.empty()) return LSSPA_OK;
  TRY(sync_all(ctx));
  for (auto& r : ctx->prof_recs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.beg, r.end) == hipSuccess) {
      ctx->prof_ms[r.cls] += ms;
      ctx->prof_n[r.cls] += 1;
    }
    (void)hipEventDestroy(r.beg);
    (void)hipEventDestroy(r.end);
  }
  ctx->prof_recs.clear();
  return LSSPA_OK;
}

// ---- small helper kernels that only the API layer needs ---------------------------------
template <typename T>
__global__ void transpose_test_kernel(const T* __restrict__ X, const T* __restrict__ y, int64_t M, int64_t ld,
                                      int p, int m_pad, double* __restrict__ Ft, double* __restrict__ ytil) {
  // Ft[f][r] = X[r][f]; tiny (M < p), clarity over speed
  const int64_t total = (int64_t)p * m_pad;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
    const int f = (int)(o / m_pad), r = (int)(o - (int64_t)f * m_pad);
    Ft[o] = (r < M) ? (double)X[(int64_t)r * ld + f] : 0.0;
  }
  if (blockIdx.x == 0)
    for (int r = threadIdx.x; r < m_pad; r += 256) ytil[r] = (r < M) ? (double)y[r] : 0.0;
}

__global__ void sumsq_kernel(const double* __restrict__ v, int n, double* __restrict__ out) {
  __shared__ double s[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += v[i] * v[i];
  s[threadIdx.x] = a;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) s[threadIdx.x] += s[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = s[0];
}

// ---- problem set-up -----------------------------------------------------------------------
// Drop the per-batch workspace (it is re-created on demand).  The capacities are zeroed FIRST, so that a context
// whose next allocation fails is left with "no workspace", never with a capacity that points at freed buffers.
void free_lane_workspace(Lane& L) {
  L.cap_ord = 0;
  L.cap_samples = 0;
  L.perms_used_valid[0] = L.perms_used_valid[1] = false;
  dev_free(L.A);
  dev_free(L.V);
  dev_free(L.Dinv);
  dev_free(L.diag0);
  dev_free(L.Ppart);
  dev_free(L.run);
  dev_free(L.row_flags);
  dev_free(L.perms_d);
  dev_free(L.lifts);
  dev_free(L.folded);
}

void free_workspace(lsspa_ctx* ctx) {
  for (Lane& L : ctx->lanes) free_lane_workspace(L);
  dev_free(ctx->stat_parts);
}

// wait for everything this context has in flight: the lanes' streams and the context's own
int sync_all(lsspa_ctx* ctx) {
  for (Lane& L : ctx->lanes) {
    if (L.st) HIPCHK(hipStreamSynchronize(L.st));
    if (L.copy_stream) HIPCHK(hipStreamSynchronize(L.copy_stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return LSSPA_OK;
}

int set_dims(lsspa_ctx* ctx, int p, int m, int tri) {
  if (p < 1 || m < 1) return ctx->fail(LSSPA_ERR_ARG, "p and m must be positive");
  if (tri && m != p) return ctx->fail(LSSPA_ERR_ARG, "tri mode needs m == p");
  if (p > max_features()) {
    // the reference has no limit (ls_spa/ls_spa.py:163); here one work matrix of p_pad^2 elements is indexed with 32
    // bits in places.  Refused now, by name, rather than at the first batch's launch.  (Up to round 3 the limit was
    // 13567: a source row and the ordering had to fit the LDS of a CU; the segmented gather lifted that.)
    char msg[160];
    snprintf(msg, sizeof msg, "p = %d features exceeds the %d this engine supports (32-bit element counts of one "
             "p x p work matrix)", p, max_features());
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  TRY(sync_all(ctx));  // buffers below may be re-allocated
  ctx->have_problem = false;
  ctx->r2_valid = false;
  ctx->min_rel_pivot = 1.0;
  ctx->src_f32_valid = false;
  ctx->g_players = 0;   // a player map belongs to the problem it was set on
  ctx->pairs_on = false;   // ... and so does the pair state: its dimension is the sample's
  // a workspace sized for another shape is released now: kept, it would count as unavailable memory when the
  // new one is sized from hipMemGetInfo (and its layout depends on p_pad / m_pad / tri anyway)
  for (Lane& L : ctx->lanes) L.in_flight = false;   // a batch launched on the previous problem is void
  if (p != ctx->p || m != ctx->m || tri != ctx->tri) {
    free_workspace(ctx);
    dev_free(ctx->Gf);
    dev_free(ctx->Hf);
  }
  ctx->p = p;
  ctx->m = m;
  ctx->tri = tri;
  ctx->p_pad = work_p_pad(p);
  ctx->m_pad = round_up(m, 128);
  const size_t pp = (size_t)ctx->p_pad;
  TRY(dev_alloc(ctx, ctx->G, (size_t)p * pp));
  TRY(dev_alloc(ctx, ctx->g, pp));
  TRY(dev_alloc(ctx, ctx->scal, 8));
  if (tri) {
    TRY(dev_alloc(ctx, ctx->H, (size_t)p * pp));
    TRY(dev_alloc(ctx, ctx->h, pp));
  } else {
    TRY(dev_alloc(ctx, ctx->Ft, (size_t)p * ctx->m_pad));
    TRY(dev_alloc(ctx, ctx->ytil, (size_t)ctx->m_pad));
  }
  TRY(dev_alloc(ctx, ctx->mean, (size_t)p));
  TRY(dev_alloc(ctx, ctx->M2, (size_t)p * p));
  TRY(dev_alloc(ctx, ctx->pend, (size_t)1 + p + (size_t)p * p));
  TRY(dev_alloc(ctx, ctx->state_n, 8));
  TRY(dev_alloc(ctx, ctx->mean_alt, (size_t)p));
  TRY(dev_alloc(ctx, ctx->state_alt, 8));
  TRY(dev_alloc(ctx, ctx->info_d, 8));
  // so does the lift history (row stride): it has to be enabled again for the new problem
  ctx->hist_cap = 0;
  ctx->hist_n = 0;
  ctx->run_on = false;
  return LSSPA_OK;
}

int stats_reset(lsspa_ctx* ctx) {
  const int p = ctx->p;
  HIPCHK(hipMemsetAsync(ctx->mean.ptr, 0, sizeof(double) * p, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->M2.ptr, 0, sizeof(double) * (size_t)p * p, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->pend.ptr, 0, sizeof(double) * ((size_t)1 + p + (size_t)p * p), ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->state_n.ptr, 0, sizeof(double) * 8, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->state_alt.ptr, 0, sizeof(double) * 8, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->info_d.ptr, 0, sizeof(int32_t) * 8, ctx->stream));
  ctx->pend_dirty = false;
  ctx->hist_n = 0;
  if (ctx->run_on) {
    HIPCHK(hipMemsetAsync(ctx->Dacc.ptr, 0, ctx->Dacc.count * 8, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->sacc.ptr, 0, ctx->sacc.count * 8, ctx->stream));
    for (bool& v : ctx->res_valid) v = false;
  }
  return LSSPA_OK;
}

// append rows [rows][sd] (device or host, row stride sd = the sample dimension) to the history
int hist_append(lsspa_ctx* ctx, const double* src, int64_t rows, hipMemcpyKind kind) {
  const size_t ldh = ctx->ldh();
  if (ctx->hist_n + rows > ctx->hist_cap) {
    // grow geometrically; the capacity given to lsspa_history_enable is only the first allocation
    const int64_t cap = std::max<int64_t>(2 * ctx->hist_cap, ctx->hist_n + rows);
    const int64_t cap_rows = ((cap + KCH - 1) / KCH) * KCH;
    DevBuf<double> bigger;
    TRY(dev_alloc(ctx, bigger, (size_t)cap_rows * ldh));
    HIPCHK(hipMemsetAsync(bigger.ptr, 0, bigger.count * 8, ctx->stream));
    if (ctx->hist_n > 0)
      HIPCHK(hipMemcpyAsync(bigger.ptr, ctx->hist.ptr, (size_t)ctx->hist_n * ldh * 8, hipMemcpyDeviceToDevice,
                            ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    dev_free(ctx->hist);
    ctx->hist = bigger;
    ctx->hist_cap = cap;
  }
  HIPCHK(hipMemcpy2DAsync(ctx->hist.ptr + (size_t)ctx->hist_n * ldh, ldh * 8, src, (size_t)ctx->sd() * 8,
                          (size_t)ctx->sd() * 8, (size_t)rows, kind, ctx->stream));
  ctx->hist_n += rows;
  return LSSPA_OK;
}

// elements of one ordering's V buffer: V row-major (strip kernel) or, in tri mode, V^T as a chunk-major p_pad x p_pad
// matrix (X tiles of the panel launches) -- room for either, so that developer flag 128 can switch between them
size_t v_elems_per_ordering(const lsspa_ctx* ctx) {
  const size_t rowmajor = (size_t)v_rows_of(ctx->p) * (size_t)ldv_of(ctx->m_pad);
  const size_t pp = ctx->p_pad;
  return ctx->tri ? std::max(rowmajor, pp * pp) : rowmajor;
}

// tri mode computes V^T inside the panel launches; rect mode (and developer flag 128) uses the strip kernel
static inline bool vt_path(const lsspa_ctx* ctx) { return vt_rule(ctx->tri, ctx->flags); }
// the X tiles scan their own blocks of V^T for the lifts (developer flag 512: the lift kernel reads V^T back instead)
static inline bool fused_scan(const lsspa_ctx* ctx) { return vt_path(ctx) && !(ctx->flags & 512); }

size_t bytes_per_ordering(const lsspa_ctx* ctx) {
  const size_t pp = ctx->p_pad, nblk = pp / NB;
  const size_t nm = ctx->tri ? 2 : 1;
  const size_t es = ctx->esz();
  // work matrices, V / V^T, inverse diagonal blocks, initial diagonals, partial sums, lift vector; the fused scan's
  // running sums and row flags; the two device copies of the ordering
  return nm * pp * pp * es + v_elems_per_ordering(ctx) * es +
         nm * nblk * 4096 * es + nm * pp * 8 +
         (size_t)(ctx->m_pad / 64) * pp * 8 + (size_t)ctx->p * 8 +
         pp * 8 + 2 * sizeof(int32_t) + 2 * (size_t)ctx->p * sizeof(int32_t);
}

int ensure_workspace(lsspa_ctx* ctx, Lane& L, int want_ord, int want_samples) {
  want_ord = (want_ord + 1) & ~1;  // antithetical pairs stay together
  if (want_ord > L.cap_ord || want_samples > L.cap_samples)
    TRY(sync_all(ctx));  // work in flight still uses the old buffers
  if (want_ord > L.cap_ord) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    // memory already held by the old workspace comes back when it is re-allocated
    const size_t per = bytes_per_ordering(ctx);
    size_t budget = (size_t)(0.85 * (double)free_b) + (size_t)L.cap_ord * per;
    if (ctx->n_lanes == 2 && &L == &ctx->lanes[0] && ctx->lanes[1].cap_ord == 0)
      budget /= 2;   // leave the second lane its share
    int cap = (int)std::min<size_t>((size_t)want_ord, budget / per);
    cap = std::min(cap, 4096);
    cap &= ~1;  // keep antithetical pairs together
    if (cap < 2) return ctx->fail(LSSPA_ERR_NOMEM, "not enough device memory for two orderings");
    if (cap > L.cap_ord) {
      // capacity 0 while the buffers are being replaced: if one allocation fails (LSSPA_ERR_NOMEM) the caller may
      // retry with a smaller batch and must then find "no workspace", not the old capacity over freed buffers
      const int samples_kept = L.cap_samples;
      DevBuf<double> lifts_kept = L.lifts;
      L.lifts = DevBuf<double>();
      free_lane_workspace(L);
      L.lifts = lifts_kept;
      L.cap_samples = samples_kept;
      const size_t pp = ctx->p_pad, nblk = pp / NB;
      const size_t nm = ctx->tri ? 2 : 1;
      const size_t es = ctx->esz();
      TRY(dev_alloc(ctx, L.A, nm * cap * pp * pp * es));
      TRY(dev_alloc(ctx, L.V, (size_t)cap * v_elems_per_ordering(ctx) * es));
      TRY(dev_alloc(ctx, L.Dinv, nm * cap * nblk * 4096 * es));
      TRY(dev_alloc(ctx, L.diag0, nm * cap * pp));
      TRY(dev_alloc(ctx, L.Ppart, (size_t)cap * (ctx->m_pad / 64) * pp));
      if (ctx->tri) {
        TRY(dev_alloc(ctx, L.run, (size_t)cap * pp));
        TRY(dev_alloc(ctx, L.row_flags, (size_t)2 * cap));
      }
      TRY(dev_alloc(ctx, L.perms_d, (size_t)2 * cap * ctx->p));
      L.cap_ord = cap;
    }
  }
  if (want_samples > L.cap_samples) {
    L.cap_samples = 0;   // dev_alloc releases the old buffer before it asks for the new one
    TRY(dev_alloc(ctx, L.lifts, (size_t)want_samples * ctx->p));
    L.cap_samples = want_samples;
  }
  return LSSPA_OK;
}

// player map set: the lane's [samples][g] buffer of group lifts (the fold's output)
int ensure_folded(lsspa_ctx* ctx, Lane& L, int want_samples) {
  const size_t need = (size_t)want_samples * ctx->g_players;
  if (L.folded.ptr && L.folded.count >= need) return LSSPA_OK;
  TRY(sync_all(ctx));  // work in flight still uses the old buffer
  return dev_alloc(ctx, L.folded, need);
}

// what a launched batch hands to collect: its lift vectors [B][p], or -- player map set -- its group lifts [B][g]
static inline const double* lane_out(const lsspa_ctx* ctx, const Lane& L) {
  return ctx->g_players ? L.folded.ptr : L.lifts.ptr;
}
// player map with a baseline: an antithetical sample's two orderings run as two unpaired orderings (rows 2 s and
// 2 s + 1 of the lift buffer, averaged by the fold).  The kernels' paired form takes ordering 2 s + 1 to be ordering 2 s
// read backwards, which expands the reversed group ordering only when no baseline has to stay in front.
static inline bool split_pairs(const lsspa_ctx* ctx, int per_sample) {
  return ctx->g_players && per_sample == 2 && !ctx->players.base.empty();
}

int ensure_pinned(lsspa_ctx* ctx, Lane& L, size_t count) {
  if (L.perms_h_count >= count) return LSSPA_OK;
  TRY(sync_all(ctx));  // pending copies still read the old buffers
  L.perms_h_count = 0;
  for (int b = 0; b < 2; ++b) {
    if (L.perms_h[b]) (void)hipHostFree(L.perms_h[b]);
    L.perms_h[b] = nullptr;
    L.perms_busy[b] = false;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&L.perms_h[b]), count * sizeof(int32_t), 0);
    if (e != hipSuccess) return ctx->fail(LSSPA_ERR_NOMEM, "hipHostMalloc", e);
    if (!L.perms_ev[b]) HIPCHK(hipEventCreateWithFlags(&L.perms_ev[b], hipEventDisableTiming));
  }
  L.perms_h_count = count;
  return LSSPA_OK;
}

// streams and events of a lane, made on first use
int ensure_lane(lsspa_ctx* ctx, Lane& L) {
  if (!L.ev_done) {
    HIPCHK(hipEventCreateWithFlags(&L.ev_mid, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&L.ev_done, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&L.ev_consumed, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&L.ev_main, hipEventDisableTiming));
  }
  if (ctx->n_lanes == 2 && !L.st) HIPCHK(hipStreamCreateWithFlags(&L.st, hipStreamNonBlocking));
  return LSSPA_OK;
}

// The lifts of a sample telescope to R^2 up to the round-off of the Gram / Cholesky route, c p eps / (smallest relative
// pivot): 1e-9 (fp64) covers that while the smallest relative pivot the full fit met stays 1e6 times above the NOT_PD
// threshold 16 p eps; below that the tolerance grows with 1 / pivot, so that what ill-conditioned data do to a correct
// engine (measured: DESIGN.md, Numerics) is not reported as a fault of the engine.  At the NOT_PD threshold itself
// it has reached 1e-3.  fp32 work: the fixed 1e-4 (its threshold is within 1e3 of a well-conditioned pivot already).
static double sum_check_tol(const lsspa_ctx* ctx) {
  if (ctx->f32 || ctx->r2_f32) return 1e-4 * std::max(1.0, std::fabs(ctx->r2));
  const double piv_tol = 16.0 * (double)ctx->p * 2.220446049250313e-16;
  const double cond = (ctx->min_rel_pivot > 0.0) ? 1e6 * piv_tol / ctx->min_rel_pivot : 1.0;
  return 1e-9 * std::max(1.0, std::fabs(ctx->r2)) * std::min(1e6, std::max(1.0, cond));
}

// small problems take the fused kernel (developer flag 1024 forces the general path, which full_fit, get_factors and
// debug_factor also need: they read the factors back from the work matrices)
static bool small_path(const lsspa_ctx* ctx) {
  return ctx->tri && !ctx->f32 && small_p_eligible(ctx->p) && !(ctx->flags & 1024) && !ctx->general_path_once;
}

// Run gather -> factorisation -> strip -> lift for n_ord orderings already resident in perms_d.
// lifts for sample s land in lifts_d[(s_off + s)][p].
// Orderings [ord_off, ord_off + n_ord) of the staged batch on stream st.  Each slice owns its part of every
// workspace buffer (a slice's matrices are laid out [source][ordering] inside its own region), so two
// slices can run on two streams at once.
int run_slice(lsspa_ctx* ctx, Lane& L, int ord_off, int n_ord, int per_sample, int s_off, hipStream_t st) {
  const int p = ctx->p, p_pad = ctx->p_pad, m_pad = ctx->m_pad, nblk = p_pad / NB;
  const int n_src = ctx->tri ? 2 : 1;
  const int n_mats = n_ord * n_src;
  const size_t es = ctx->esz(), pp2 = (size_t)p_pad * p_pad;
  char* const A_s = L.A.ptr + (size_t)ord_off * n_src * pp2 * es;
  char* const Dinv_s = L.Dinv.ptr + (size_t)ord_off * n_src * nblk * 4096 * es;
  double* const diag0_s = L.diag0.ptr + (size_t)ord_off * n_src * p_pad;
  char* const V_s = L.V.ptr + (size_t)ord_off * v_elems_per_ordering(ctx) * es;
  const bool vt = vt_path(ctx);   // V^T by the panel launches' X tiles instead of the strip kernel
  double* const Ppart_s = L.Ppart.ptr + (size_t)ord_off * (m_pad / 64) * p_pad;
  const int32_t* const perms_s = L.perms_cur + (size_t)ord_off * p;
  const bool timed = (st == ctx->lane_stream(L));   // the profiling events live on the lane's main stream
  // a1: small problems take the fused kernel (developer flag 1024 forces the general path, which full_fit,
  // get_factors and debug_factor also need: they read the factors back from the work matrices)
  if (small_path(ctx)) {
    ProfScope ps(timed ? ctx : nullptr, LSSPA_K_SMALL, st);
    SmallArgs sa;
    sa.S[0] = ctx->G.ptr;
    sa.S[1] = ctx->H.ptr;
    sa.s[0] = ctx->g.ptr;
    sa.s[1] = ctx->h.ptr;
    sa.aug[0] = 2.0 * ctx->aug_train + 1.0;
    sa.aug[1] = 2.0 * ctx->y_norm_sq + 1.0;
    sa.ld_src = p_pad;
    sa.fwd_only = (L.perms_fwd_only && per_sample == 2) ? 1 : 0;
    sa.perms = sa.fwd_only ? L.perms_cur + (size_t)(ord_off / 2) * p : perms_s;
    sa.p = p;
    sa.nb = (p + 1 + 15) / 16;
    sa.n_ord = n_ord;
    sa.per_sample = per_sample;
    sa.lifts = L.lifts.ptr + (size_t)s_off * p;
    sa.y_norm_sq = ctx->y_norm_sq;
    sa.piv_tol = 16.0 * (double)p * 2.220446049250313e-16;
    sa.info = ctx->info_d.ptr;
    sa.variant = (ctx->flags & 16384) ? 1 : 0;
    // the batch's own end-to-end check (run_orderings) inside the kernel where the kernel can make it
    sa.r2 = ctx->r2;
    sa.sum_tol = -1.0;
    sa.sum_quiet = 0.0;
    L.sum_checked = false;
    if (ctx->r2_valid && small_p_checks_sum(sa)) {
      sa.sum_tol = sum_check_tol(ctx);
      L.sum_checked = true;
    }
    if (per_sample == 2)
      HIPCHK(hipMemsetAsync(sa.lifts, 0, sizeof(double) * (size_t)(n_ord / 2) * p, st));
    HIPCHK(launch_small_p(sa, st));
    return LSSPA_OK;
  }
  {
    ProfScope ps(timed ? ctx : nullptr, LSSPA_K_GATHER, st);
    GatherArgs ga;
    ga.S[0] = ctx->G.ptr;
    ga.s[0] = ctx->g.ptr;
    ga.aug[0] = 2.0 * ctx->aug_train + 1.0;
    ga.S[1] = ctx->tri ? ctx->H.ptr : nullptr;
    ga.s[1] = ctx->tri ? ctx->h.ptr : nullptr;
    ga.aug[1] = 2.0 * ctx->y_norm_sq + 1.0;
    ga.Sf[0] = ga.Sf[1] = nullptr;
    if (ctx->f32) {   // made by ensure_f32_sources() before the first slice is launched
      ga.Sf[0] = ctx->Gf.ptr;
      ga.Sf[1] = ctx->tri ? ctx->Hf.ptr : nullptr;
    }
    ga.ld_src = p_pad;
    ga.perms = perms_s;
    ga.p = p;
    ga.p_pad = p_pad;
    ga.n_ord = n_ord;
    ga.n_src = n_src;
    ga.A = A_s;
    ga.diag0 = diag0_s;
    ga.f32 = ctx->f32;
    ga.paired = (per_sample == 2) ? 1 : 0;   // stage_and_run lays pairs out back to back
    HIPCHK(launch_gather(ga, st));
  }
  // a pivot below ~p ulps of its feature's own variance is numerically zero (collinear feature)
  const double piv_tol = 16.0 * (double)p * (ctx->f32 ? 1.1920929e-07 : 2.220446049250313e-16);
  {
    ProfScope ps(timed ? ctx : nullptr, LSSPA_K_CHOL_DIAG, st);
    // (the diagonal launch also zeroes the fused lift scan's row flags of its matrices)
    HIPCHK(launch_chol2_diag(A_s, Dinv_s, diag0_s, piv_tol, ctx->info_d.ptr, p_pad, n_mats, ctx->f32, st,
                             fused_scan(ctx) ? L.row_flags.ptr + (size_t)ord_off * n_src : nullptr));
  }
  const int n_launch = panel_launches(p_pad, vt);
  PanelLift pl;
  pl.mode = 0;
  if (fused_scan(ctx)) {
    pl.flags = L.row_flags.ptr + (size_t)ord_off * n_src;
    pl.run = L.run.ptr + (size_t)ord_off * p_pad;
    pl.Ppart = Ppart_s;
    pl.pstride = (int64_t)(m_pad / 64) * p_pad;
    pl.p = p;
    // the factors themselves are wanted (debug_factor reads V^T back): keep the last panel's stores
    pl.mode = ctx->general_path_once ? 1 : 2;
  }
  for (int Jo = 0; Jo < n_launch; ++Jo) {
    {
      ProfScope ps(timed ? ctx : nullptr, LSSPA_K_CHOL_PANEL, st);
      HIPCHK(launch_chol2_panel(A_s, Dinv_s, diag0_s, piv_tol, ctx->info_d.ptr, p_pad, Jo, n_mats, ctx->f32, st,
                                ctx->flags, work_p_live(p), vt ? V_s : nullptr, n_ord, pl.mode ? &pl : nullptr));
    }
    // two lanes: the other lane's next batch may start once this one is about half done
    // (the hand-over point scanned at the C3 shape, round 4, eight launches: after launch 0 / 1 / 2 / 3 / 4 / 5 / 6 / 7 ->
    // 6.32 / 6.33 / 6.29 / 6.25 / 6.32 / 6.39 / 6.40 / 6.48 ms per step, one lane 6.44-6.52)
    // (with two half-batches per step on the two lanes, 20 steps: after launch 1 / 2 / 3 / 4 / 5 -> 6.24 / 6.22 / 6.19 /
    // 6.28 / 6.38 ms)
    static const int handover_env = [] { const char* e = getenv("LSSPA_HANDOVER"); return e ? atoi(e) : -1; }();
    const int handover = handover_env >= 0 ? std::min(handover_env, n_launch - 1) : std::max(0, n_launch / 2 - 1);
    if (L.mid_armed && timed && Jo == handover) {
      HIPCHK(hipEventRecord(L.ev_mid, st));
      L.mid_valid = true;
      L.mid_armed = false;
    }
  }
  if (!vt) {
    ProfScope ps(timed ? ctx : nullptr, LSSPA_K_STRIP, st);
    StripArgs sa;
    sa.A = A_s;
    sa.Dinv = Dinv_s;
    sa.rhs = ctx->tri ? A_s + (size_t)n_ord * pp2 * es : nullptr;
    sa.Ft = ctx->tri ? nullptr : ctx->Ft.ptr;
    sa.f32 = ctx->f32;
    sa.perms = perms_s;
    sa.V = V_s;
    sa.p = p;
    sa.p_pad = p_pad;
    sa.m_pad = m_pad;
    sa.n_ord = n_ord;
    sa.tri = ctx->tri;
    sa.flags = ctx->flags;
    sa.row_live = work_p_live(p);
    sa.col_live = ctx->tri ? work_p_live(p) : round_up(ctx->m, 16);
    HIPCHK(launch_strip(sa, st));
  }
  {
    ProfScope ps(timed ? ctx : nullptr, LSSPA_K_LIFT, st);
    LiftArgs la;
    la.A = A_s;
    la.At = ctx->tri ? A_s + (size_t)n_ord * pp2 * es : nullptr;
    la.f32 = ctx->f32;
    la.ytil = ctx->tri ? nullptr : ctx->ytil.ptr;
    la.V = V_s;
    la.vt = vt ? 1 : 0;
    la.fused = pl.mode ? 1 : 0;
    la.perms = perms_s;
    la.Ppart = Ppart_s;
    la.lifts = L.lifts.ptr + (size_t)s_off * p;
    la.y_norm_sq = ctx->y_norm_sq;
    la.p = p;
    la.p_pad = p_pad;
    la.m_pad = m_pad;
    la.n_ord = n_ord;
    la.per_sample = per_sample;
    la.tri = ctx->tri;
    la.paired = (per_sample == 2) ? 1 : 0;   // stage_and_run builds the second ordering as the reverse of the first
    HIPCHK(launch_lift(la, st));
  }
  return LSSPA_OK;
}

// the problem (or a derived copy of it) changed on the context's stream: lanes order themselves behind this point
int mark_problem(lsspa_ctx* ctx) {
  if (!ctx->ev_problem) HIPCHK(hipEventCreateWithFlags(&ctx->ev_problem, hipEventDisableTiming));
  HIPCHK(hipEventRecord(ctx->ev_problem, ctx->stream));
  ++ctx->problem_epoch;
  return LSSPA_OK;
}

// fp32 mode: the gather reads fp32 copies of the Gram matrices.  Converted once per problem on the context's
// stream, BEFORE a batch forks onto a second stream (a slice on the side stream must not race the conversion).
int ensure_f32_sources(lsspa_ctx* ctx) {
  if (!ctx->f32 || ctx->src_f32_valid) return LSSPA_OK;
  const size_t cnt = (size_t)ctx->p * ctx->p_pad;
  TRY(dev_alloc(ctx, ctx->Gf, cnt));
  HIPCHK(launch_to_f32(ctx->G.ptr, ctx->Gf.ptr, (int64_t)cnt, ctx->stream));
  if (ctx->tri) {
    TRY(dev_alloc(ctx, ctx->Hf, cnt));
    HIPCHK(launch_to_f32(ctx->H.ptr, ctx->Hf.ptr, (int64_t)cnt, ctx->stream));
  }
  ctx->src_f32_valid = true;
  return mark_problem(ctx);
}

// Run gather -> factorisation (with V^T) -> lift for n_ord orderings already resident in perms_d.
// lifts for sample s land in lifts_d[(s_off + s)][p].  (Rounds 1-3 could cut a batch into two slices on two streams of
// ONE lane, developer flag 32, +0.8 %; the two lanes of round 4 do that across batches and better -- removed.)
int run_orderings(lsspa_ctx* ctx, Lane& L, int n_ord, int per_sample, int s_off) {
  const hipStream_t st = ctx->lane_stream(L);
  L.sum_checked = false;
  TRY(run_slice(ctx, L, 0, n_ord, per_sample, s_off, st));
  // the batch's own end-to-end check, once the full model's R^2 is known (lsspa_full_fit): every lift vector sums to it
  // (the register-resident small-problem kernel has made it per ordering already)
  if (ctx->r2_valid && !ctx->general_path_once && !L.sum_checked)
    HIPCHK(launch_sum_check(L.lifts.ptr + (size_t)s_off * ctx->p, n_ord / per_sample, ctx->p, ctx->r2, sum_check_tol(ctx),
                            ctx->info_d.ptr, st));
  return LSSPA_OK;
}

// Stage `count` orderings (with their reverses when per_sample == 2) on lane L and run them.  Player map set: perms
// are [n_samples][g] orderings of the groups, expanded to column orderings as they are staged, and the batch's last
// launch folds its lift vectors into group lifts (lane_out).
int stage_and_run(lsspa_ctx* ctx, Lane& L, const int32_t* perms, int n_samples, int per_sample, int s_off) {
  const int p = ctx->p;
  const int n_ord = n_samples * per_sample;
  const int grp = ctx->g_players;
  const bool split = split_pairs(ctx, per_sample);
  const int kper = split ? 1 : per_sample;          // orderings per sample as the kernels see them
  const int row_off = split ? 2 * s_off : s_off;    // the batch's first row of the lane's lift buffer
  const hipStream_t st = ctx->lane_stream(L);
  const int turn = L.perms_turn;
  L.perms_turn ^= 1;
  if (L.perms_busy[turn]) {  // the copy that last read this buffer must have run
    HIPCHK(hipEventSynchronize(L.perms_ev[turn]));
    L.perms_busy[turn] = false;
  }
  // ... and, where uploads go by the copy stream, the kernels that read the device slot two batches ago must have
  // finished: the host's lead over the GPU stays at two batches a lane.  (A copy on its own stream is done long before
  // its batch starts, so the wait above no longer holds the host back -- and a host five groups ahead of a one-lane
  // C2 run met a 7 ms stall inside the runtime at its fifth launch: 128 steps 0.075 ms each against 0.029 for 64.)
  if (L.perms_used_valid[turn]) HIPCHK(hipEventSynchronize(L.perms_used[turn]));
  int32_t* hp = L.perms_h[turn];
  // the small-problem kernels read a sample's reverse ordering out of the forward one themselves: half the staging, half
  // the upload (the host's share of a 2048-ordering group at p = 100 was longer than the GPU's)
  L.perms_fwd_only = kper == 2 && small_path(ctx);
  if (grp) {
    const int stride = L.perms_fwd_only ? 1 : per_sample;
    for (int s = 0; s < n_samples; ++s) {
      const int32_t* src = perms + (size_t)s * grp;
      int32_t* d0 = hp + (size_t)s * stride * p;
      expand_group_row(ctx->players, src, 0, d0);
      if (stride == 2) {
        int32_t* d1 = d0 + p;
        if (split) expand_group_row(ctx->players, src, 1, d1);
        else for (int j = 0; j < p; ++j) d1[j] = d0[p - 1 - j];
      }
    }
  } else if (L.perms_fwd_only || per_sample == 1) {
    std::memcpy(hp, perms, sizeof(int32_t) * (size_t)n_samples * p);   // validated by the caller
  } else {
    for (int s = 0; s < n_samples; ++s) {
      const int32_t* src = perms + (size_t)s * p;
      int32_t* d0 = hp + (size_t)s * 2 * p;
      std::memcpy(d0, src, sizeof(int32_t) * (size_t)p);
      int32_t* d1 = d0 + p;
      for (int j = 0; j < p; ++j) d1[j] = src[p - 1 - j];
    }
  }
  // the kernels of the batch, then (player map) the fold of rows [row_off ..) into group lifts [s_off ..)
  auto run = [&]() -> int {
    TRY(run_orderings(ctx, L, n_ord, kper, row_off));
    if (!grp) return LSSPA_OK;
    ProfScope ps(ctx, LSSPA_K_LIFT, st);
    HIPCHK(launch_fold_players(L.lifts.ptr + (size_t)row_off * p, p, split ? 2 : 1, ctx->pl_off.ptr, ctx->pl_cols.ptr, grp,
                               n_samples, L.folded.ptr + (size_t)s_off * grp, st));
    return LSSPA_OK;
  };
  int32_t* dp = L.perms_d.ptr + (size_t)turn * L.cap_ord * p;
  const size_t bytes = sizeof(int32_t) * (size_t)(L.perms_fwd_only ? n_samples : n_ord) * p;
  if (bytes <= ((size_t)256 << 10) || (ctx->n_lanes == 2 && bytes <= ((size_t)1 << 20))) {
    // a small upload rides on the lane's own stream: one copy and one event (the pinned buffer's reuse guard)
    // instead of a hand-off to the copy stream and back -- four stream operations that cost the host more than
    // the copy costs the GPU.  With two lanes that holds up to 1 MB (the other lane's kernels run meanwhile, and copy
    // streams beside two lanes and the context's stream are more streams than hardware queues: C3 6.70 against 5.92 ms
    // a step, measured).  With one lane only up to 256 KB: a group of 4096 orderings at p = 100 waited 36 us for its
    // own 0.8 MB between two 400 us kernels -- on the copy stream it arrives while the previous group runs.
    HIPCHK(hipMemcpyAsync(dp, hp, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(L.perms_ev[turn], st));
    L.perms_busy[turn] = true;
    L.perms_cur = dp;
    L.perms_used_valid[turn] = false;    // stream order protects the device slot
    return run();
  }
  if (!L.copy_stream) {
    HIPCHK(hipStreamCreateWithFlags(&L.copy_stream, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) HIPCHK(hipEventCreateWithFlags(&L.perms_used[b], hipEventDisableTiming));
  }
  if (L.perms_used_valid[turn]) HIPCHK(hipStreamWaitEvent(L.copy_stream, L.perms_used[turn], 0));
  HIPCHK(hipMemcpyAsync(dp, hp, bytes, hipMemcpyHostToDevice, L.copy_stream));
  HIPCHK(hipEventRecord(L.perms_ev[turn], L.copy_stream));
  L.perms_busy[turn] = true;
  HIPCHK(hipStreamWaitEvent(st, L.perms_ev[turn], 0));
  L.perms_cur = dp;
  const int rc = run();
  if (rc != LSSPA_OK) return rc;
  HIPCHK(hipEventRecord(L.perms_used[turn], st));
  L.perms_used_valid[turn] = true;
  return LSSPA_OK;
}

// Launch a batch on the next lane: every kernel up to the lift vectors.  Nothing here touches the running statistics,
// so a batch can be launched before the previous one has been accumulated (or is ever accumulated: lift_discard).
int lift_launch(lsspa_ctx* ctx, const int32_t* perms, int B, int per, Lane** out) {
  const int p = ctx->p;
  Lane& L = ctx->lanes[ctx->n_lanes == 2 ? ctx->lane_turn : 0];
  if (L.in_flight) return ctx->fail(LSSPA_ERR_STATE, "both lanes hold a launched batch: collect or discard one first");
  TRY(ensure_lane(ctx, L));
  TRY(ensure_f32_sources(ctx));   // on the context's stream ...
  // orderings per launch sequence: everything at once up to ~8 GB of workspace or 4096 orderings
  const size_t per_ord = bytes_per_ordering(ctx);
  const int want = (int)std::max<size_t>(2, std::min<size_t>(4096, ((size_t)8 << 30) / per_ord));
  TRY(ensure_workspace(ctx, L, std::min(B * per, std::max(want, 512)), split_pairs(ctx, per) ? 2 * B : B));
  if (ctx->g_players) TRY(ensure_folded(ctx, L, B));
  const int sub = std::max(1, L.cap_ord / per);
  TRY(ensure_pinned(ctx, L, (size_t)std::min(sub, (int)B) * per * p));
  const hipStream_t st = ctx->lane_stream(L);
  if (ctx->n_lanes == 2) {
    Lane& other = ctx->lanes[1 - ctx->lane_turn];
    // ... which the lane's stream has to see (fp32 sources, a freshly loaded problem, a reset)
    if (L.problem_seen != ctx->problem_epoch) {
      // NOT an event recorded now: the context's stream already holds the statistics of the previous batch, which
      // wait for that batch's kernels -- waiting on "now" would chain this batch behind the whole previous one
      HIPCHK(hipStreamWaitEvent(st, ctx->ev_problem, 0));
      L.problem_seen = ctx->problem_epoch;
    }
    // this lane's previous lift vectors have been read by the statistics
    if (L.consumed_valid) HIPCHK(hipStreamWaitEvent(st, L.ev_consumed, 0));
    // stagger: start when the other lane's batch is half way
    if (other.mid_valid) HIPCHK(hipStreamWaitEvent(st, other.ev_mid, 0));
    L.mid_armed = true;
  }
  for (int s0 = 0; s0 < B; s0 += sub) {
    const int ns = std::min(sub, B - s0);
    TRY(stage_and_run(ctx, L, perms + (size_t)s0 * ctx->sd(), ns, per, s0));
  }
  if (ctx->n_lanes == 2) {
    if (L.mid_armed) {   // one-level path or a single panel: no mid point was met
      HIPCHK(hipEventRecord(L.ev_mid, st));
      L.mid_valid = true;
      L.mid_armed = false;
    }
    HIPCHK(hipEventRecord(L.ev_done, st));
    L.done_valid = true;
    ctx->lane_turn ^= 1;
  }
  L.B = B;
  L.per = per;
  L.taken = 0;
  L.in_flight = true;
  ctx->lane_last = (int)(&L - ctx->lanes);
  if (out) *out = &L;
  return LSSPA_OK;
}

// accumulate: 0 = lift vectors only, 1 = fold into the pending buffer, 2 = fold and merge at once.  2 is a one-GPU
// short cut: refused while a batch is pending (its moments are about another mean) and on a context whose
// communicator spans several ranks (the merge would use per-rank statistics).  Checked BEFORE anything is enqueued.
int check_accumulate(lsspa_ctx* ctx, int accumulate) {
  if (accumulate < 0 || accumulate > 2) return ctx->fail(LSSPA_ERR_ARG, "accumulate must be 0, 1 or 2");
  if (accumulate == 2 && ctx->pend_dirty)
    return ctx->fail(LSSPA_ERR_STATE, "accumulate = 2 (fold and merge at once) with a batch pending: merge it first");
  if (accumulate == 2 && ctx->comm && comm_world(ctx->comm) > 1)
    return ctx->fail(LSSPA_ERR_STATE, "accumulate = 2 (fold and merge at once) on a context with a multi-rank "
                                      "communicator: the moments must be all-reduced before the merge");
  return LSSPA_OK;
}

// Fold `count` samples of a launched batch, from sample `first` on, into the pending statistics (accumulate) and /
// or copy their lift vectors out -- on the context's stream, in order.  The parts of a batch are taken front to
// back; the lane is given back with the last one.
// What becomes of a collected chunk's lift vectors beyond the statistics: appended to the history (the thin-form
// estimator, or the running form's staging until lsspa_error_advance names their sample ids) or, when the caller knows
// the ids already (lsspa_group_collect), folded into the running estimator's sums straight from the lane's buffer.
int keep_lifts(lsspa_ctx* ctx, const double* src, int count, const int64_t* ids /* first_id, stride or null */) {
  if (ctx->run_on && ids) {
    const int n_pad = ((count + KCH - 1) / KCH) * KCH;
    TRY(dev_alloc(ctx, ctx->xi_d, (size_t)ERR_DRAWS * n_pad));
    ProfScope ps(ctx, LSSPA_K_ERROR);
    HIPCHK(launch_error_accumulate(ctx->run_seed, ids[0], ids[1], count, n_pad, ctx->xi_d.ptr, src, ctx->sd(), 1,
                                   ctx->ldh(), ctx->sd(), ctx->Dacc.ptr, ctx->sacc.ptr, ctx->stream));
    return LSSPA_OK;
  }
  if (ctx->hist_cap > 0) TRY(hist_append(ctx, src, count, hipMemcpyDeviceToDevice));
  return LSSPA_OK;
}

int lane_taken(lsspa_ctx* ctx, Lane& L, int upto);

int lift_collect(lsspa_ctx* ctx, Lane& L, int first, int count, double* lifts_out, int accumulate,
                 const int64_t* est_ids = nullptr) {
  if (!L.in_flight) return ctx->fail(LSSPA_ERR_STATE, "no launched batch on this lane");
  const int p = ctx->sd();   // a sample's dimension: g with a player map
  if (count <= 0) count = L.B - first;
  if (first != L.taken || count < 1 || first + count > L.B)
    return ctx->fail(LSSPA_ERR_ARG, "parts of a launched batch are collected front to back, without gaps");
  TRY(check_accumulate(ctx, accumulate));   // before the stream is touched: a refused call leaves the lane as it was
  const double* src = lane_out(ctx, L) + (size_t)first * p;
  if (ctx->n_lanes == 2 && first == 0) HIPCHK(hipStreamWaitEvent(ctx->stream, L.ev_done, 0));
  if (accumulate == 2 && stats_small_fusable(count, p)) {
    // single GPU, small p: moments and merge in ONE launch; the advanced mean and n land in the other halves of the
    // pairs, which then become the current ones
    ProfScope ps(ctx, LSSPA_K_STATS);
    HIPCHK(launch_stats_small_fused(src, ctx->mean.ptr, ctx->state_n.ptr, ctx->mean_alt.ptr, ctx->state_alt.ptr,
                                    ctx->M2.ptr, count, p, ctx->stream));
    std::swap(ctx->mean, ctx->mean_alt);
    std::swap(ctx->state_n, ctx->state_alt);
    TRY(keep_lifts(ctx, src, count, est_ids));
  } else if (accumulate) {
    {
      ProfScope ps(ctx, LSSPA_K_STATS);
      const int nz = stats_batch_slices(count, p);
      if (nz > 1) TRY(dev_alloc(ctx, ctx->stat_parts, (size_t)nz * ((size_t)1 + p + (size_t)p * p)));
      HIPCHK(launch_stats_batch(src, ctx->mean.ptr, ctx->pend.ptr, count, p, ctx->pend_dirty ? 1 : 0,
                                nz > 1 ? ctx->stat_parts.ptr : nullptr, ctx->stream));
      ctx->pend_dirty = true;
    }
    TRY(keep_lifts(ctx, src, count, est_ids));
    if (accumulate == 2) TRY(lsspa_stats_merge(ctx));   // the general path: the same effect in its usual launches
  }
  if (lifts_out) {
    HIPCHK(hipMemcpyAsync(lifts_out, src, sizeof(double) * (size_t)count * p, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  return lane_taken(ctx, L, first + count);
}

// Small problems, one rank: the statistics of SEVERAL chunks of a launched batch in one launch (stats_small_multi_kernel),
// chunk by chunk in order -- bit for bit what lift_collect(accumulate = 2) does chunk after chunk.  The chunks follow
// each other in the batch (first[c + 1] = first[c] + count[c]).  snap: keep the running mean and n after every chunk
// (ctx->mean_snap / n_snap) for the checks that belong to them.  The caller has checked fusability (chunks_fusable).
bool chunks_fusable(const lsspa_ctx* ctx, const Lane& L, int n_chunks, const int32_t* first, const int32_t* count) {
  if (ctx->comm || ctx->pend_dirty || n_chunks < 2 || n_chunks > StatsChunks::MAX || !L.in_flight) return false;
  if (first[0] != L.taken) return false;
  int next = first[0];
  for (int c = 0; c < n_chunks; ++c) {
    if (first[c] != next || !stats_small_fusable(count[c], ctx->sd())) return false;
    next += count[c];
  }
  return next <= L.B;
}

int collect_chunks_small(lsspa_ctx* ctx, Lane& L, int n_chunks, const int32_t* first, const int32_t* count,
                                bool snap) {
  const int p = ctx->sd();
  if (ctx->n_lanes == 2 && first[0] == 0) HIPCHK(hipStreamWaitEvent(ctx->stream, L.ev_done, 0));
  StatsChunks ch;
  ch.n = n_chunks;
  for (int c = 0; c < n_chunks; ++c) {
    ch.first[c] = first[c];
    ch.count[c] = count[c];
  }
  if (snap) {
    TRY(dev_alloc(ctx, ctx->mean_snap, (size_t)StatsChunks::MAX * p));
    TRY(dev_alloc(ctx, ctx->n_snap, (size_t)StatsChunks::MAX));
  }
  {
    ProfScope ps(ctx, LSSPA_K_STATS);
    HIPCHK(launch_stats_small_multi(lane_out(ctx, L), ctx->mean.ptr, ctx->state_n.ptr, ctx->mean_alt.ptr, ctx->state_alt.ptr,
                                    ctx->M2.ptr, ch, p, snap ? ctx->mean_snap.ptr : nullptr,
                                    snap ? ctx->n_snap.ptr : nullptr, ctx->stream));
  }
  std::swap(ctx->mean, ctx->mean_alt);
  std::swap(ctx->state_n, ctx->state_alt);
  return LSSPA_OK;
}

// what lift_collect does to the lane when the last sample of its batch has been taken
int lane_taken(lsspa_ctx* ctx, Lane& L, int upto) {
  L.taken = upto;
  if (L.taken == L.B) {
    if (ctx->n_lanes == 2) {
      HIPCHK(hipEventRecord(L.ev_consumed, ctx->stream));
      L.consumed_valid = true;
    }
    L.in_flight = false;
  }
  return LSSPA_OK;
}

bool is_permutation(const int32_t* perm, int p, std::vector<char>& seen) {
  seen.assign(p, 0);
  for (int j = 0; j < p; ++j) {
    const int32_t f = perm[j];
    if (f < 0 || f >= p || seen[f]) return false;
    seen[f] = 1;
  }
  return true;
}

// No exception crosses the C ABI: std::vector / std::string / new inside an entry point turn into a status code
// (an escaping std::bad_alloc would be std::terminate, i.e. an abort of the host process).
int abi_caught(lsspa_ctx* ctx) noexcept {
  const char* what = "C++ exception inside the library";
  int code = LSSPA_ERR_HIP;
  try {
    throw;
  } catch (const std::bad_alloc&) {
    what = "out of host memory";
    code = LSSPA_ERR_NOMEM;
  } catch (const std::exception& e) {
    what = e.what();
  } catch (...) {
  }
  try {
    if (ctx) ctx->err = what;
    else g_create_error = what;
  } catch (...) {
  }
  return code;
}

}  // namespace

// =============================================================================================
extern "C" {

int lsspa_abi_version(void) { return LSSPA_ABI_VERSION; }

const char* lsspa_last_error(const lsspa_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int lsspa_create(int32_t device, lsspa_ctx** out) {
  if (!out) {
    g_create_error = "out pointer is NULL";
    return LSSPA_ERR_ARG;
  }
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n < 1) {
    g_create_error = std::string("no HIP device available: ") + hipGetErrorString(e);
    return LSSPA_ERR_HIP;
  }
  if (device < 0 || device >= n) {
    g_create_error = "device index out of range";
    return LSSPA_ERR_ARG;
  }
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) {
    g_create_error = std::string("hipGetDeviceProperties: ") + hipGetErrorString(e);
    return LSSPA_ERR_HIP;
  }
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    g_create_error = std::string("this library is built for gfx950 only, device is ") + prop.gcnArchName;
    return LSSPA_ERR_HIP;
  }
  lsspa_ctx* ctx = new (std::nothrow) lsspa_ctx();
  if (!ctx) {
    g_create_error = "out of host memory";
    return LSSPA_ERR_NOMEM;
  }
  ctx->device = device;
  if (prop.multiProcessorCount > 0) ctx->n_cu = prop.multiProcessorCount;
  if ((e = hipSetDevice(device)) != hipSuccess ||
      (e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) {
    g_create_error = std::string("stream creation: ") + hipGetErrorString(e);
    delete ctx;
    return LSSPA_ERR_HIP;
  }
  ctx->own_stream = true;
  // The two lanes' streams NOW, second and third of the context: the runtime deals its few hardware queues to streams
  // in the order they are made, and a lane that lands on the queue of the context's stream waits behind the statistics
  // that wait for the other lane -- the lanes then run one after the other.  Made on first use they came after the
  // streamed reduction's copy stream: the public call at C3, alone in a process, 38.0 k orderings/s against 41.7 k
  // with this order (round 5, tools/full_run_probe.py; bench.py's own engine never streams a reduction and never saw it).
  for (int k = 0; k < 2; ++k)
    if ((e = hipStreamCreateWithFlags(&ctx->lanes[k].st, hipStreamNonBlocking)) != hipSuccess) {
      g_create_error = std::string("stream creation: ") + hipGetErrorString(e);
      for (int j = 0; j < k; ++j) (void)hipStreamDestroy(ctx->lanes[j].st);
      (void)hipStreamDestroy(ctx->stream);
      delete ctx;
      return LSSPA_ERR_HIP;
    }
  *out = ctx;
  return LSSPA_OK;
}

int lsspa_destroy(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_OK;
  (void)hipSetDevice(ctx->device);
  (void)sync_all(ctx);
  for (auto& r : ctx->prof_recs) {
    (void)hipEventDestroy(r.beg);
    (void)hipEventDestroy(r.end);
  }
  dev_free(ctx->G); dev_free(ctx->g); dev_free(ctx->H); dev_free(ctx->h); dev_free(ctx->Ft);
  dev_free(ctx->ytil); dev_free(ctx->scal); dev_free(ctx->info_d);
  dev_free(ctx->mean); dev_free(ctx->M2); dev_free(ctx->pend); dev_free(ctx->state_n);
  dev_free(ctx->mean_alt); dev_free(ctx->state_alt);
  dev_free(ctx->Cred);
  dev_free(ctx->Gf); dev_free(ctx->Hf);
  ctx->sub.release();
  ctx->grp.release();
  ctx->boot.release();
  ctx->cv.release();
  ctx->multi.release();
  ctx->mlift.release();
  ctx->cvlift.release();
  ctx->bootlift.release();
  ctx->perm.release();
  dev_free(ctx->pl_off); dev_free(ctx->pl_cols);
  dev_free(ctx->pr_count); dev_free(ctx->pr_mean); dev_free(ctx->pr_m2); dev_free(ctx->pr_phi);
  dev_free(ctx->pr_delta); dev_free(ctx->pr_lifts); dev_free(ctx->pr_pos); dev_free(ctx->pr_perms);
  if (ctx->pr_perms_h) (void)hipHostFree(ctx->pr_perms_h);
  if (ctx->pr_ev) (void)hipEventDestroy(ctx->pr_ev);
  free_workspace(ctx);
  for (Lane& L : ctx->lanes) {
    if (L.copy_stream) {
      (void)hipStreamDestroy(L.copy_stream);
      for (int b = 0; b < 2; ++b) (void)hipEventDestroy(L.perms_used[b]);
    }
    if (L.ev_done) {
      (void)hipEventDestroy(L.ev_mid);
      (void)hipEventDestroy(L.ev_done);
      (void)hipEventDestroy(L.ev_consumed);
      (void)hipEventDestroy(L.ev_main);
    }
    if (L.st) (void)hipStreamDestroy(L.st);
    for (int b = 0; b < 2; ++b) {
      if (L.perms_h[b]) (void)hipHostFree(L.perms_h[b]);
      if (L.perms_ev[b]) (void)hipEventDestroy(L.perms_ev[b]);
    }
  }
  dev_free(ctx->hist); dev_free(ctx->xi_d); dev_free(ctx->draws); dev_free(ctx->err_out);
  dev_free(ctx->Dacc); dev_free(ctx->sacc);
  if (ctx->res_h) (void)hipHostFree(ctx->res_h);
  for (hipEvent_t& e : ctx->res_ev)
    if (e) (void)hipEventDestroy(e);
  if (ctx->ev_problem) (void)hipEventDestroy(ctx->ev_problem);
  comm_destroy(ctx->comm);
  ctx->comm = nullptr;
  dev_free(ctx->pack); dev_free(ctx->xfer); dev_free(ctx->ibuf); dev_free(ctx->theta_d);
  dev_free(ctx->mean_snap); dev_free(ctx->n_snap);
  dev_free(ctx->grp_P); dev_free(ctx->grp_S); dev_free(ctx->grp_D); dev_free(ctx->grp_s); dev_free(ctx->grp_norms);
  for (int b = 0; b < 2; ++b) {
    dev_free(ctx->red_x[b]);
    dev_free(ctx->red_y[b]);
    if (ctx->red_copied[b]) (void)hipEventDestroy(ctx->red_copied[b]);
    if (ctx->red_consumed[b]) (void)hipEventDestroy(ctx->red_consumed[b]);
  }
  if (ctx->red_cs) (void)hipStreamDestroy(ctx->red_cs);
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_set_stream(lsspa_ctx* ctx, void* hip_stream) try {
  if (!ctx) return LSSPA_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  TRY(sync_all(ctx));
  if (hip_stream) {
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
    ctx->own_stream = false;
  } else if (!ctx->own_stream) {
    HIPCHK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    ctx->own_stream = true;
  }
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_synchronize(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  return sync_all(ctx);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_set_lanes(lsspa_ctx* ctx, int32_t n) try {
  if (!ctx || (n != 1 && n != 2)) return LSSPA_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  for (const Lane& L : ctx->lanes)
    if (L.in_flight) return ctx->fail(LSSPA_ERR_STATE, "a launched batch is still to be collected");
  TRY(sync_all(ctx));
  if (n == 1) free_lane_workspace(ctx->lanes[1]);   // the second workspace goes back to the pool
  ctx->n_lanes = n;
  ctx->lane_turn = 0;
  for (Lane& L : ctx->lanes) {
    L.mid_valid = L.done_valid = L.consumed_valid = false;
    L.problem_seen = -1;
  }
  if (n == 2 && !ctx->ev_problem) TRY(mark_problem(ctx));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

// ---------------------------------------------------------------------------------------------
// C (device, [P1pad][P1pad], P1pad = round_up(p + 1, 128)) = [X | y]^T [X | y] over the n rows given
static int gram_side(lsspa_ctx* ctx, const void* X, const void* y, int64_t n, int64_t ld, int p, int is_f32,
                     double* C_out) {
  const int n_split = gram_default_split(n, p);
  DevBuf<double> slabs, C;
  C.ptr = C_out;
  int rc = dev_alloc(ctx, slabs, gram_workspace_bytes(p, n_split) / sizeof(double));
  if (rc == LSSPA_OK) {
    ProfScope ps(ctx, LSSPA_K_GRAM);
    GramArgs ga;
    ga.X = X;
    ga.y = y;
    ga.n = n;
    ga.ld = ld;
    ga.p = p;
    ga.is_f32 = is_f32;
    ga.slabs = slabs.ptr;
    ga.n_split = n_split;
    ga.C = C.ptr;
    ga.accumulate = 0;
    ga.variant = (ctx->flags >> 16) & 0xff;
    hipError_t e = launch_gram(ga, ctx->stream);
    if (e != hipSuccess) rc = ctx->fail(LSSPA_ERR_HIP, "gram launch", e);
  }
  if (rc == LSSPA_OK) {
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = ctx->fail(LSSPA_ERR_HIP, "gram sync", e);
  }
  dev_free(slabs);
  return rc;
}

// Gram of a HOST-resident [n][ld] matrix, streamed: the rows cross PCIe in chunks through two device
// buffers on a copy stream while the previous chunk's Gram runs on the compute stream; the chunk
// Grams accumulate in C in chunk order.  The copies read the caller's pageable memory through the runtime's ordinary
// path: the caller's pages are never page-locked (rounds 2-3 registered them in place; measured slower -- registering
// 2 x 800 MB cost 14-21 ms to save about 10 ms of copy time -- and it was the one code path that touched memory it did
// not own; removed in round 4).
static int gram_side_streamed(lsspa_ctx* ctx, const void* X, const void* y, int64_t n, int64_t ld, int p,
                              int is_f32, double* C_out) {
  const size_t es = is_f32 ? 4 : 8;
  int64_t rows = (((int64_t)96 << 20) / ((int64_t)p * (int64_t)es) / 16) * 16;   // ~96 MB chunks
  rows = std::max<int64_t>(1024, std::min<int64_t>(rows, ((n + 15) / 16) * 16));
  if (ctx->red_chunk_rows > 0) rows = ctx->red_chunk_rows;   // test hook: many short chunks from a small matrix
  const int n_split = gram_default_split(rows, p);
  DevBuf<double> slabs, C;
  void* dX[2] = {nullptr, nullptr};
  void* dy[2] = {nullptr, nullptr};
  hipStream_t cs = nullptr;
  hipEvent_t copied[2] = {nullptr, nullptr}, consumed[2] = {nullptr, nullptr};
  C.ptr = C_out;
  int rc = dev_alloc(ctx, slabs, gram_workspace_bytes(p, n_split) / sizeof(double));
  hipError_t e = hipSuccess;
  if (rc == LSSPA_OK) {
    // the staging buffers, the copy stream and the events live with the context: made on first use, found in place by
    // the second side of this reduction and by the next call (four hipMalloc / hipFree pairs of ~100 MB per call before)
    for (int b = 0; b < 2 && rc == LSSPA_OK; ++b) {
      rc = dev_alloc(ctx, ctx->red_x[b], (size_t)rows * p * es);
      if (rc == LSSPA_OK) rc = dev_alloc(ctx, ctx->red_y[b], (size_t)rows * es);
      if (rc == LSSPA_OK && !ctx->red_copied[b]) e = hipEventCreateWithFlags(&ctx->red_copied[b], hipEventDisableTiming);
      if (rc == LSSPA_OK && e == hipSuccess && !ctx->red_consumed[b])
        e = hipEventCreateWithFlags(&ctx->red_consumed[b], hipEventDisableTiming);
      dX[b] = ctx->red_x[b].ptr;
      dy[b] = ctx->red_y[b].ptr;
      copied[b] = ctx->red_copied[b];
      consumed[b] = ctx->red_consumed[b];
    }
    if (rc == LSSPA_OK && e == hipSuccess && !ctx->red_cs) e = hipStreamCreateWithFlags(&ctx->red_cs, hipStreamNonBlocking);
    cs = ctx->red_cs;
    if (rc == LSSPA_OK && e != hipSuccess) rc = ctx->fail(LSSPA_ERR_NOMEM, "streamed reduction buffers", e);
  }
  const auto t_stream0 = std::chrono::steady_clock::now();
  auto seconds_since = [](std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  };
  if (rc == LSSPA_OK) {
    ProfScope ps(ctx, LSSPA_K_GRAM);
    int k = 0;
    for (int64_t r0 = 0; r0 < n && e == hipSuccess; r0 += rows, ++k) {
      const int b = k & 1;
      const int64_t nr = std::min<int64_t>(rows, n - r0);
      if (k >= 2) e = hipStreamWaitEvent(cs, consumed[b], 0);   // the Gram of chunk k-2 has read this buffer
      const char* src = static_cast<const char*>(X) + (size_t)r0 * ld * es;
      if (e == hipSuccess) {
        if (ld == p)
          e = hipMemcpyAsync(dX[b], src, (size_t)nr * p * es, hipMemcpyHostToDevice, cs);
        else
          e = hipMemcpy2DAsync(dX[b], (size_t)p * es, src, (size_t)ld * es, (size_t)p * es, (size_t)nr,
                               hipMemcpyHostToDevice, cs);
      }
      if (e == hipSuccess)
        e = hipMemcpyAsync(dy[b], static_cast<const char*>(y) + (size_t)r0 * es, (size_t)nr * es,
                           hipMemcpyHostToDevice, cs);
      if (e == hipSuccess) e = hipEventRecord(copied[b], cs);
      if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, copied[b], 0);
      if (e == hipSuccess) {
        GramArgs ga;
        ga.X = dX[b];
        ga.y = dy[b];
        ga.n = nr;
        ga.ld = p;
        ga.p = p;
        ga.is_f32 = is_f32;
        ga.slabs = slabs.ptr;
        ga.n_split = n_split;
        ga.C = C.ptr;
        ga.accumulate = k > 0;
        ga.variant = (ctx->flags >> 16) & 0xff;
        e = launch_gram(ga, ctx->stream);
      }
      if (e == hipSuccess) e = hipEventRecord(consumed[b], ctx->stream);
    }
    if (e != hipSuccess) rc = ctx->fail(LSSPA_ERR_HIP, "streamed gram", e);
  }
  // Both streams are idle before the buffers go -- on the error paths too: every copy
  // that reads the caller's pages was enqueued on cs, every kernel that reads dX / dy on the context's stream.
  hipError_t es1 = hipStreamSynchronize(ctx->stream);
  hipError_t es2 = cs ? hipStreamSynchronize(cs) : hipSuccess;
  if (rc == LSSPA_OK && es1 != hipSuccess) rc = ctx->fail(LSSPA_ERR_HIP, "streamed gram sync", es1);
  if (rc == LSSPA_OK && es2 != hipSuccess) rc = ctx->fail(LSSPA_ERR_HIP, "streamed gram copy sync", es2);
  ctx->red_stream_s += seconds_since(t_stream0);
  dev_free(slabs);
  return rc;
}

// The local part of the reduction: unscaled Gram sums of this context's rows into ctx->Cred
// ([2][P1pad][P1pad]: train, test), or -- rect mode, test side -- the transposed test factor.
static int reduce_rows(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* y_train, int64_t N,
                       const void* X_test, int64_t ld_test, const void* y_test, int64_t M, int32_t p,
                       int32_t dtype, int32_t location, int tri) {
  const size_t es = dtype == LSSPA_F32 ? 4 : 8;
  const int is_f32 = dtype == LSSPA_F32;
  const size_t c_elems = (size_t)round_up(p + 1, 128) * round_up(p + 1, 128);
  ctx->red_stream_s = ctx->red_finalize_s = 0.0;
  TRY(dev_alloc(ctx, ctx->Cred, 2 * c_elems));
  HIPCHK(hipMemsetAsync(ctx->Cred.ptr, 0, 2 * c_elems * 8, ctx->stream));
  auto side = [&](const void* X, const void* y, int64_t n, int64_t ld, bool train) -> int {
    if (n == 0) return LSSPA_OK;   // a rank without rows on this side contributes zeros
    double* C = ctx->Cred.ptr + (train ? 0 : c_elems);
    if (location == LSSPA_HOST && (train || tri)) return gram_side_streamed(ctx, X, y, n, ld, p, is_f32, C);
    if (train || tri) return gram_side(ctx, X, y, n, ld, p, is_f32, C);
    // rect mode: F = X_test as it stands (M < p rows), stored transposed; ||y_test||^2 on the side
    const void *dX = X, *dy = y;
    void *tX = nullptr, *ty = nullptr;
    int64_t dld = ld;
    int rc = LSSPA_OK;
    if (location == LSSPA_HOST) {
      hipError_t e = hipMalloc(&tX, (size_t)n * p * es);
      if (e == hipSuccess) e = hipMalloc(&ty, (size_t)n * es);
      if (e != hipSuccess) {
        if (tX) (void)hipFree(tX);
        return ctx->fail(LSSPA_ERR_NOMEM, "device copy of the data", e);
      }
      e = hipMemcpy2DAsync(tX, (size_t)p * es, X, (size_t)ld * es, (size_t)p * es, (size_t)n,
                           hipMemcpyHostToDevice, ctx->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(ty, y, (size_t)n * es, hipMemcpyHostToDevice, ctx->stream);
      if (e != hipSuccess) rc = ctx->fail(LSSPA_ERR_HIP, "H2D copy of the data", e);
      dX = tX;
      dy = ty;
      dld = p;
    }
    if (rc == LSSPA_OK) {
      const int64_t total = (int64_t)p * ctx->m_pad;
      const int grid = (int)std::min<int64_t>((total + 255) / 256, 2048);
      if (is_f32)
        hipLaunchKernelGGL(transpose_test_kernel<float>, dim3(grid), dim3(256), 0, ctx->stream, (const float*)dX,
                           (const float*)dy, n, dld, p, ctx->m_pad, ctx->Ft.ptr, ctx->ytil.ptr);
      else
        hipLaunchKernelGGL(transpose_test_kernel<double>, dim3(grid), dim3(256), 0, ctx->stream,
                           (const double*)dX, (const double*)dy, n, dld, p, ctx->m_pad, ctx->Ft.ptr,
                           ctx->ytil.ptr);
      hipLaunchKernelGGL(sumsq_kernel, dim3(1), dim3(256), 0, ctx->stream, ctx->ytil.ptr, ctx->m_pad,
                         ctx->scal.ptr + 1);
      hipError_t e = hipGetLastError();
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
      if (e != hipSuccess) rc = ctx->fail(LSSPA_ERR_HIP, "test factor kernels", e);
    }
    if (tX) (void)hipFree(tX);
    if (ty) (void)hipFree(ty);
    return rc;
  };
  TRY(side(X_train, y_train, N, ld_train, true));
  TRY(side(X_test, y_test, M, ld_test, false));
  return LSSPA_OK;
}

// G = C_train / N + reg I, g, (tri) H = C_test, h, ||y_test||^2 from the summed Gram buffers
static int reduce_finalize(lsspa_ctx* ctx, int64_t N_total, double reg) {
  const int p = ctx->p;
  const auto t_fin0 = std::chrono::steady_clock::now();
  struct Stop {
    lsspa_ctx* c;
    std::chrono::steady_clock::time_point t0;
    ~Stop() { c->red_finalize_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
  } stop{ctx, t_fin0};
  const size_t c_elems = (size_t)round_up(p + 1, 128) * round_up(p + 1, 128);
  // (not part of the LSSPA_K_GRAM timing class: that class counts the Gram contractions, one launch per side)
  HIPCHK(launch_gram_finalize(ctx->Cred.ptr, p, 1.0 / (double)N_total, reg, ctx->G.ptr, ctx->p_pad, ctx->g.ptr,
                              ctx->scal.ptr + 0, ctx->stream));
  if (ctx->tri)
    HIPCHK(launch_gram_finalize(ctx->Cred.ptr + c_elems, p, 1.0, 0.0, ctx->H.ptr, ctx->p_pad, ctx->h.ptr,
                                ctx->scal.ptr + 1, ctx->stream));
  double sc[2];
  HIPCHK(hipMemcpyAsync(sc, ctx->scal.ptr, sizeof sc, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->aug_train = sc[0];
  ctx->y_norm_sq = sc[1];
  if (!(ctx->y_norm_sq > 0.0)) return ctx->fail(LSSPA_ERR_ARG, "y_test is identically zero (or NaN)");
  TRY(stats_reset(ctx));
  ctx->have_problem = true;
  TRY(mark_problem(ctx));
  ctx->reduce_open = false;
  dev_free(ctx->Cred);
  return LSSPA_OK;
}

int lsspa_reduce(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* y_train, int64_t N,
                 const void* X_test, int64_t ld_test, const void* y_test, int64_t M, int32_t p, double reg,
                 int32_t dtype, int32_t location) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!X_train || !y_train || !X_test || !y_test) return ctx->fail(LSSPA_ERR_ARG, "NULL data pointer");
  if (p < 1 || N < p || M < 1 || ld_train < p || ld_test < p)
    return ctx->fail(LSSPA_ERR_ARG, "need 1 <= p <= N, M >= 1, ld >= p");
  if (dtype != LSSPA_F64 && dtype != LSSPA_F32) return ctx->fail(LSSPA_ERR_ARG, "dtype");
  if (location != LSSPA_HOST && location != LSSPA_DEVICE) return ctx->fail(LSSPA_ERR_ARG, "location");
  if (!(reg >= 0.0)) return ctx->fail(LSSPA_ERR_ARG, "reg must be >= 0");
  HIPCHK(hipSetDevice(ctx->device));
  const int tri = (M >= p) ? 1 : 0;
  if (!tri && M > (1 << 20)) return ctx->fail(LSSPA_ERR_ARG, "M too large for rect mode");
  TRY(set_dims(ctx, p, tri ? p : (int)M, tri));
  TRY(reduce_rows(ctx, X_train, ld_train, y_train, N, X_test, ld_test, y_test, M, p, dtype, location, tri));
  return reduce_finalize(ctx, N, reg);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_reduce_timing(const lsspa_ctx* ctx, double* seconds4) {
  if (!ctx || !seconds4) return LSSPA_ERR_ARG;
  seconds4[0] = 0.0;
  seconds4[1] = ctx->red_stream_s;
  seconds4[2] = 0.0;
  seconds4[3] = ctx->red_finalize_s;
  return LSSPA_OK;
}

int lsspa_reduce_partial(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* y_train,
                         int64_t n_local, const void* X_test, int64_t ld_test, const void* y_test,
                         int64_t m_local, int64_t M_total, int32_t p, int32_t dtype, int32_t location) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (n_local < 0 || m_local < 0 || M_total < 1 || m_local > M_total || p < 1)
    return ctx->fail(LSSPA_ERR_ARG, "need n_local >= 0, 0 <= m_local <= M_total, p >= 1");
  if ((n_local > 0 && (!X_train || !y_train || ld_train < p)) || (m_local > 0 && (!X_test || !y_test || ld_test < p)))
    return ctx->fail(LSSPA_ERR_ARG, "NULL data pointer or ld < p");
  if (dtype != LSSPA_F64 && dtype != LSSPA_F32) return ctx->fail(LSSPA_ERR_ARG, "dtype");
  if (location != LSSPA_HOST && location != LSSPA_DEVICE) return ctx->fail(LSSPA_ERR_ARG, "location");
  HIPCHK(hipSetDevice(ctx->device));
  const int tri = (M_total >= p) ? 1 : 0;
  if (!tri && m_local != M_total)
    return ctx->fail(LSSPA_ERR_ARG, "M_total < p: the test rows are the factor itself, pass all of them on every rank");
  if (!tri && M_total > (1 << 20)) return ctx->fail(LSSPA_ERR_ARG, "M too large for rect mode");
  TRY(set_dims(ctx, p, tri ? p : (int)M_total, tri));
  TRY(reduce_rows(ctx, X_train, ld_train, y_train, n_local, X_test, ld_test, y_test, m_local, p, dtype, location,
                  tri));
  ctx->reduce_open = true;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_reduce_buffer(lsspa_ctx* ctx, void** device_ptr, int64_t* count) try {
  if (!ctx || !device_ptr || !count) return LSSPA_ERR_ARG;
  if (!ctx->reduce_open) return ctx->fail(LSSPA_ERR_STATE, "no partial reduction in progress");
  *device_ptr = ctx->Cred.ptr;
  const int64_t P1pad = round_up(ctx->p + 1, 128);
  *count = 2 * P1pad * P1pad;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_reduce_finish(lsspa_ctx* ctx, int64_t N_total, double reg) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!ctx->reduce_open) return ctx->fail(LSSPA_ERR_STATE, "no partial reduction in progress");
  if (N_total < ctx->p) return ctx->fail(LSSPA_ERR_ARG, "need N_total >= p");
  if (!(reg >= 0.0)) return ctx->fail(LSSPA_ERR_ARG, "reg must be >= 0");
  HIPCHK(hipSetDevice(ctx->device));
  return reduce_finalize(ctx, N_total, reg);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_set_reduced(lsspa_ctx* ctx, int32_t p, const double* G, const double* g, double aug_train,
                      int32_t tri, const double* H, const double* h, int32_t m, const double* Ft,
                      const double* ytil, double y_norm_sq) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!G || !g) return ctx->fail(LSSPA_ERR_ARG, "G and g are required");
  if (tri ? (!H || !h) : (!Ft || !ytil)) return ctx->fail(LSSPA_ERR_ARG, "test side pointers missing");
  if (!(y_norm_sq > 0.0) || !(aug_train >= 0.0)) return ctx->fail(LSSPA_ERR_ARG, "norms must be positive");
  HIPCHK(hipSetDevice(ctx->device));
  TRY(set_dims(ctx, p, tri ? p : m, tri ? 1 : 0));
  const size_t pp = ctx->p_pad;
  HIPCHK(hipMemcpy2D(ctx->G.ptr, pp * 8, G, (size_t)p * 8, (size_t)p * 8, p, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(ctx->g.ptr, 0, pp * 8));
  HIPCHK(hipMemcpy(ctx->g.ptr, g, (size_t)p * 8, hipMemcpyHostToDevice));
  if (tri) {
    HIPCHK(hipMemcpy2D(ctx->H.ptr, pp * 8, H, (size_t)p * 8, (size_t)p * 8, p, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(ctx->h.ptr, 0, pp * 8));
    HIPCHK(hipMemcpy(ctx->h.ptr, h, (size_t)p * 8, hipMemcpyHostToDevice));
  } else {
    const size_t mp = ctx->m_pad;
    HIPCHK(hipMemset(ctx->Ft.ptr, 0, (size_t)p * mp * 8));
    HIPCHK(hipMemcpy2D(ctx->Ft.ptr, mp * 8, Ft, (size_t)m * 8, (size_t)m * 8, p, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(ctx->ytil.ptr, 0, mp * 8));
    HIPCHK(hipMemcpy(ctx->ytil.ptr, ytil, (size_t)m * 8, hipMemcpyHostToDevice));
  }
  ctx->aug_train = aug_train;
  ctx->y_norm_sq = y_norm_sq;
  TRY(stats_reset(ctx));
  ctx->have_problem = true;
  TRY(mark_problem(ctx));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_get_problem(const lsspa_ctx* ctx, int32_t* p, int32_t* m, int32_t* tri, double* y_norm_sq) try {
  if (!ctx || !ctx->have_problem) return LSSPA_ERR_STATE;
  if (p) *p = ctx->p;
  if (m) *m = ctx->m;
  if (tri) *tri = ctx->tri;
  if (y_norm_sq) *y_norm_sq = ctx->y_norm_sq;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(const_cast<lsspa_ctx*>(ctx));
}

int lsspa_get_gram(lsspa_ctx* ctx, double* G, double* g, double* H, double* h) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const size_t p = ctx->p, pp = ctx->p_pad;
  if (G) HIPCHK(hipMemcpy2D(G, p * 8, ctx->G.ptr, pp * 8, p * 8, p, hipMemcpyDeviceToHost));
  if (g) HIPCHK(hipMemcpy(g, ctx->g.ptr, p * 8, hipMemcpyDeviceToHost));
  if ((H || h) && !ctx->tri) return ctx->fail(LSSPA_ERR_STATE, "no test Gram in rect mode");
  if (H) HIPCHK(hipMemcpy2D(H, p * 8, ctx->H.ptr, pp * 8, p * 8, p, hipMemcpyDeviceToHost));
  if (h) HIPCHK(hipMemcpy(h, ctx->h.ptr, p * 8, hipMemcpyDeviceToHost));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

// device -> host copy of `count` work-matrix elements starting at element offset `off`, as doubles
static int fetch_elems(lsspa_ctx* ctx, const char* base, size_t off, size_t count, double* dst) {
  if (!ctx->f32) {
    HIPCHK(hipMemcpy(dst, base + off * 8, count * 8, hipMemcpyDeviceToHost));
    return LSSPA_OK;
  }
  std::vector<float> tmp(count);
  HIPCHK(hipMemcpy(tmp.data(), base + off * 4, count * 4, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < count; ++i) dst[i] = (double)tmp[i];
  return LSSPA_OK;
}

// factor the identity ordering into workspace slot 0 (lifts into lifts_d row 0)
static int factor_identity(lsspa_ctx* ctx, const int32_t* perm_or_null) {
  const int p = ctx->p;
  for (const Lane& L : ctx->lanes)
    if (L.in_flight) return ctx->fail(LSSPA_ERR_STATE, "a launched batch is still to be collected");
  TRY(sync_all(ctx));
  Lane& L = ctx->lanes[0];
  TRY(ensure_lane(ctx, L));
  TRY(ensure_f32_sources(ctx));
  TRY(ensure_workspace(ctx, L, 2, 1));
  TRY(ensure_pinned(ctx, L, (size_t)2 * p));
  std::vector<int32_t> id(p);
  for (int j = 0; j < p; ++j) id[j] = perm_or_null ? perm_or_null[j] : j;
  TRY(sync_all(ctx));                       // the conversion above ran on the context's stream
  ctx->general_path_once = true;            // the callers read L back from the work matrices
  const int players_kept = ctx->g_players;  // ... and the lifts of a COLUMN ordering: a player map sits this out
  ctx->g_players = 0;
  const int rc = stage_and_run(ctx, L, id.data(), 1, 1, 0);
  ctx->g_players = players_kept;
  ctx->general_path_once = false;
  if (rc != LSSPA_OK) return rc;
  TRY(sync_all(ctx));                       // callers read results with blocking copies
  return LSSPA_OK;
}

int lsspa_full_fit(lsspa_ctx* ctx, double* theta, double* r_squared, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  HIPCHK(hipSetDevice(ctx->device));
  const int p = ctx->p;
  int32_t saved = 0, now = 0;
  TRY(sync_all(ctx));
  HIPCHK(hipMemcpy(&saved, ctx->info_d.ptr, 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(ctx->info_d.ptr, 0, 4));
  TRY(factor_identity(ctx, nullptr));
  HIPCHK(hipMemcpy(&now, ctx->info_d.ptr, 4, hipMemcpyDeviceToHost));
  saved |= now;
  HIPCHK(hipMemcpy(ctx->info_d.ptr, &saved, 4, hipMemcpyHostToDevice));
  if (info) *info = now;
  if (theta) {
    DevBuf<double>& th = ctx->theta_d;          // kept with the context (a hipMalloc / hipFree pair per call otherwise)
    TRY(dev_alloc(ctx, th, (size_t)2 * p));     // theta, and the running right-hand side when p exceeds the LDS
    hipError_t e = launch_backsolve(ctx->lanes[0].A.ptr, th.ptr, p, ctx->p_pad, ctx->f32, ctx->stream, th.ptr + p);
    if (e == hipSuccess) e = hipMemcpyAsync(theta, th.ptr, sizeof(double) * p, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return ctx->fail(LSSPA_ERR_HIP, "backsolve", e);
  }
  if (r_squared) {
    std::vector<double> l(p);
    HIPCHK(hipMemcpy(l.data(), ctx->lanes[0].lifts.ptr, sizeof(double) * p, hipMemcpyDeviceToHost));
    double s = 0.0;
    for (int j = 0; j < p; ++j) s += l[j];
    *r_squared = s;
    // the smallest relative pivot of this factorisation: the conditioning that the sum check's tolerance allows for
    DevBuf<double>& th = ctx->theta_d;
    TRY(dev_alloc(ctx, th, (size_t)2 * p));
    // (of G and, in tri mode, of H, whose factor follows the train matrix in the workspace: run_slice's layout)
    double piv = 1.0;
    for (int side = 0; side < (ctx->tri ? 2 : 1); ++side) {
      const char* A = ctx->lanes[0].A.ptr + (size_t)side * ctx->p_pad * ctx->p_pad * ctx->esz();
      hipError_t e = launch_rel_pivots(A, side ? ctx->H.ptr : ctx->G.ptr, th.ptr + p, p, ctx->p_pad, ctx->f32, ctx->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(l.data(), th.ptr + p, sizeof(double) * p, hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
      if (e != hipSuccess) return ctx->fail(LSSPA_ERR_HIP, "relative pivots", e);
      for (int j = 0; j < p; ++j) piv = (l[j] < piv) ? l[j] : piv;      // (a NaN leaves it as it is: now != 0 then)
    }
    ctx->min_rel_pivot = piv;
    // from now on every batch is checked against it (run_orderings); not after a factorisation that broke down
    ctx->r2 = s;
    ctx->r2_valid = (now == 0) && std::isfinite(s);
    ctx->r2_f32 = ctx->f32 != 0;
  }
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_get_factors(lsspa_ctx* ctx, double* R_tr, double* q_tr, double* F_te, double* q_te) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  HIPCHK(hipSetDevice(ctx->device));
  const int p = ctx->p, m = ctx->m, ppad = ctx->p_pad;
  const size_t mat = (size_t)ppad * ppad;       // chunk-major factor matrices (tiles.h: cm_off)
  TRY(factor_identity(ctx, nullptr));
  std::vector<double> L(mat);
  TRY(fetch_elems(ctx, ctx->lanes[0].A.ptr, 0, mat, L.data()));
  if (R_tr)
    for (int a = 0; a < p; ++a)
      for (int b = 0; b < p; ++b) R_tr[(size_t)a * p + b] = (b >= a) ? L[cm_off(ppad, b, a)] : 0.0;
  if (q_tr)
    for (int a = 0; a < p; ++a) q_tr[a] = L[cm_off(ppad, p, a)];
  if (ctx->tri) {
    if (F_te || q_te) {
      // slot layout of run_orderings: the test matrices follow the n_ord = 1 train matrices
      TRY(fetch_elems(ctx, ctx->lanes[0].A.ptr, mat, mat, L.data()));
      if (F_te)
        for (int a = 0; a < p; ++a)
          for (int b = 0; b < p; ++b) F_te[(size_t)a * p + b] = (b >= a) ? L[cm_off(ppad, b, a)] : 0.0;
      if (q_te)
        for (int a = 0; a < p; ++a) q_te[a] = L[cm_off(ppad, p, a)];
    }
  } else {
    if (F_te) {
      std::vector<double> Ft((size_t)p * ctx->m_pad);
      HIPCHK(hipMemcpy(Ft.data(), ctx->Ft.ptr, Ft.size() * 8, hipMemcpyDeviceToHost));
      for (int r = 0; r < m; ++r)
        for (int f = 0; f < p; ++f) F_te[(size_t)r * p + f] = Ft[(size_t)f * ctx->m_pad + r];
    }
    if (q_te) HIPCHK(hipMemcpy(q_te, ctx->ytil.ptr, sizeof(double) * m, hipMemcpyDeviceToHost));
  }
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

// ---------------------------------------------------------------------------------------------
int lsspa_lift_batch(lsspa_ctx* ctx, const int32_t* perms, int32_t B, int32_t antithetical,
                     double* lifts_out, int32_t accumulate) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  if (!perms || B < 1) return ctx->fail(LSSPA_ERR_ARG, "perms / B");
  HIPCHK(hipSetDevice(ctx->device));
  const int per = antithetical ? 2 : 1;
  // validate before anything is launched: a repeated index would make a permuted Gram singular
  if (!all_permutations(perms, B, ctx->sd(), ctx->perm_mark))
    return ctx->fail(LSSPA_ERR_ARG, ctx->g_players ? "perms: a row is not a permutation of the groups 0..g-1"
                                                   : "perms: a row is not a permutation of 0..p-1");
  TRY(check_accumulate(ctx, accumulate));   // nothing is launched for a call that cannot be collected
  Lane* L = nullptr;
  TRY(lift_launch(ctx, perms, B, per, &L));
  const int rc = lift_collect(ctx, *L, 0, B, lifts_out, accumulate);
  if (rc != LSSPA_OK && L->in_flight) {
    // the caller has no ticket for this batch: give the lane back as lsspa_lift_discard would (the message of the
    // failure stays in place)
    if (ctx->n_lanes == 2 && L->taken > 0 && hipEventRecord(L->ev_consumed, ctx->stream) == hipSuccess)
      L->consumed_valid = true;
    L->in_flight = false;
  }
  return rc;
} catch (...) {
  return abi_caught(ctx);
}

// The two halves of lsspa_lift_batch, for callers that want a batch in flight while they decide what to do with
// the previous one (the driver launches batch k+1 before it evaluates the stop rule on batch k).
int lsspa_lift_launch(lsspa_ctx* ctx, const int32_t* perms, int32_t B, int32_t antithetical, int32_t* ticket) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  if (!perms || B < 1 || !ticket) return ctx->fail(LSSPA_ERR_ARG, "perms / B / ticket");
  HIPCHK(hipSetDevice(ctx->device));
  if (!all_permutations(perms, B, ctx->sd(), ctx->perm_mark))
    return ctx->fail(LSSPA_ERR_ARG, ctx->g_players ? "perms: a row is not a permutation of the groups 0..g-1"
                                                   : "perms: a row is not a permutation of 0..p-1");
  Lane* L = nullptr;
  TRY(lift_launch(ctx, perms, B, antithetical ? 2 : 1, &L));
  *ticket = (int32_t)(L - ctx->lanes);
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_lift_collect(lsspa_ctx* ctx, int32_t ticket, int32_t first, int32_t count, double* lifts_out,
                       int32_t accumulate) try {
  if (!ctx || ticket < 0 || ticket > 1 || first < 0) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  HIPCHK(hipSetDevice(ctx->device));
  return lift_collect(ctx, ctx->lanes[ticket], first, count, lifts_out, accumulate);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_lift_collect_chunks(lsspa_ctx* ctx, int32_t ticket, int32_t first, int32_t chunk, int32_t n_chunks,
                              int32_t accumulate) try {
  if (!ctx || ticket < 0 || ticket > 1 || first < 0 || chunk < 1 || n_chunks < 1) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  HIPCHK(hipSetDevice(ctx->device));
  Lane& L = ctx->lanes[ticket];
  // everything a part could be refused for, before the first part is taken: a refused call leaves the lane as it was
  if (!L.in_flight) return ctx->fail(LSSPA_ERR_STATE, "no launched batch on this lane");
  if (first != L.taken || (int64_t)first + (int64_t)n_chunks * chunk > L.B)
    return ctx->fail(LSSPA_ERR_ARG, "parts of a launched batch are collected front to back, without gaps, inside the batch");
  TRY(check_accumulate(ctx, accumulate));
  if (accumulate == 2 && n_chunks <= StatsChunks::MAX) {
    int32_t f[StatsChunks::MAX], k[StatsChunks::MAX];
    for (int c = 0; c < n_chunks; ++c) {
      f[c] = first + c * chunk;
      k[c] = chunk;
    }
    if (chunks_fusable(ctx, L, n_chunks, f, k)) {
      TRY(check_accumulate(ctx, 2));
      TRY(collect_chunks_small(ctx, L, n_chunks, f, k, false));
      TRY(keep_lifts(ctx, lane_out(ctx, L) + (size_t)first * ctx->sd(), n_chunks * chunk, nullptr));
      return lane_taken(ctx, L, first + n_chunks * chunk);
    }
  }
  for (int c = 0; c < n_chunks; ++c) TRY(lift_collect(ctx, L, first + c * chunk, chunk, nullptr, accumulate));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_lift_discard(lsspa_ctx* ctx, int32_t ticket) try {
  if (!ctx || ticket < 0 || ticket > 1) return LSSPA_ERR_ARG;
  Lane& L = ctx->lanes[ticket];
  if (!L.in_flight) return ctx->fail(LSSPA_ERR_STATE, "no launched batch on this lane");
  if (ctx->n_lanes == 2 && L.taken > 0) {
    // part of the batch was collected: those statistics kernels, on the context's stream, still read this lane's
    // lift vectors -- the lane's next launch (on its own stream) has to wait for them as after a full collect
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipEventRecord(L.ev_consumed, ctx->stream));
    L.consumed_valid = true;
  }
  L.in_flight = false;    // its kernels run to completion in stream order; nothing reads their output
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

// Groups of columns as the players of the sampling path.  The map changes the dimension of everything a sample is
// (sd()): the statistics start over, and the history and the estimator -- whose row stride follows the dimension --
// have to be enabled again, as after a new problem.
int lsspa_set_players(lsspa_ctx* ctx, const int32_t* labels, int32_t g) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  HIPCHK(hipSetDevice(ctx->device));
  for (const Lane& L : ctx->lanes)
    if (L.in_flight) return ctx->fail(LSSPA_ERR_STATE, "a launched batch is still to be collected");
  TRY(player_map_set(ctx, "labels is NULL (clear the map with labels = NULL, g = 0)", labels, ctx->p, g,
                     [&] { return sync_all(ctx); }, ctx->players, ctx->pl_off, ctx->pl_cols, ctx->g_players));
  ctx->pairs_on = false;   // the pair state has the dimension it was enabled at
  ctx->hist_cap = 0;
  ctx->hist_n = 0;
  ctx->run_on = false;
  return stats_reset(ctx);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_expand_groups(const int32_t* labels, int32_t p, int32_t g, const int32_t* group_perms, int32_t B,
                              int32_t antithetical, int32_t* out) try {
  if (!labels || !group_perms || !out || p < 1 || B < 1) return LSSPA_ERR_ARG;
  PlayerMap map;
  if (player_map_build(labels, p, g, map)) return LSSPA_ERR_ARG;
  std::vector<int32_t> mark;
  if (!all_permutations(group_perms, B, g, mark)) return LSSPA_ERR_ARG;
  const int per = antithetical ? 2 : 1;
  for (int s = 0; s < B; ++s) {
    int32_t* d0 = out + (size_t)s * per * p;
    expand_group_row(map, group_perms + (size_t)s * g, 0, d0);
    if (per == 2) {
      // as stage_and_run lays a pair out: with a baseline the expansion of the reversed group ordering (run unpaired),
      // without one the forward row read backwards (the kernels' paired form)
      if (!map.base.empty()) expand_group_row(map, group_perms + (size_t)s * g, 1, d0 + p);
      else for (int j = 0; j < p; ++j) d0[p + j] = d0[p - 1 - j];
    }
  }
  return LSSPA_OK;
} catch (...) {
  return abi_caught(nullptr);
}

// ---------------------------------------------------------------------------------------------
// Sampled pairwise interaction index (include/lsspa.h, lsspa_pairs_*; csrc/k_pairs.hip)
namespace {

int pairs_zero(lsspa_ctx* ctx) {
  const size_t d = (size_t)ctx->pairs_d;
  HIPCHK(hipMemsetAsync(ctx->pr_count.ptr, 0, d * d * sizeof(int64_t), ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->pr_mean.ptr, 0, d * d * 8, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->pr_m2.ptr, 0, d * d * 8, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->pr_phi.ptr, 0, d * 8, ctx->stream));
  ctx->pairs_n = 0;
  return LSSPA_OK;
}

int pairs_usable(lsspa_ctx* ctx) {
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  if (!ctx->pairs_on || ctx->pairs_d != ctx->sd())
    return ctx->fail(LSSPA_ERR_STATE, "the pair state is off: call lsspa_pairs_enable (a reduction, lsspa_set_reduced "
                                      "and lsspa_set_players switch it off)");
  return LSSPA_OK;
}

// the orderings of a batch on the device (pinned staging, no wait for the stream) and the per-batch buffers
int pairs_stage(lsspa_ctx* ctx, const int32_t* perms, int B) {
  const size_t d = (size_t)ctx->pairs_d, cnt = (size_t)B * d;
  if (ctx->pr_delta.count < cnt || ctx->pr_pos.count < cnt || ctx->pr_perms.count < cnt)
    HIPCHK(hipStreamSynchronize(ctx->stream));   // the previous batch's pair kernels still use the old buffers
  TRY(dev_alloc(ctx, ctx->pr_delta, cnt));
  TRY(dev_alloc(ctx, ctx->pr_pos, cnt));
  TRY(dev_alloc(ctx, ctx->pr_perms, cnt));
  if (!ctx->pr_ev) HIPCHK(hipEventCreateWithFlags(&ctx->pr_ev, hipEventDisableTiming));
  if (ctx->pr_ev_busy) {
    HIPCHK(hipEventSynchronize(ctx->pr_ev));
    ctx->pr_ev_busy = false;
  }
  if (ctx->pr_perms_h_count < cnt) {
    if (ctx->pr_perms_h) (void)hipHostFree(ctx->pr_perms_h);
    ctx->pr_perms_h = nullptr;
    ctx->pr_perms_h_count = 0;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&ctx->pr_perms_h), cnt * sizeof(int32_t), 0);
    if (e != hipSuccess) return ctx->fail(LSSPA_ERR_NOMEM, "hipHostMalloc", e);
    ctx->pr_perms_h_count = cnt;
  }
  std::memcpy(ctx->pr_perms_h, perms, cnt * sizeof(int32_t));
  // on the context's stream, behind the previous batch's pair kernels (which read pr_perms)
  HIPCHK(hipMemcpyAsync(ctx->pr_perms.ptr, ctx->pr_perms_h, cnt * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipEventRecord(ctx->pr_ev, ctx->stream));
  ctx->pr_ev_busy = true;
  return LSSPA_OK;
}

int pairs_kernels(lsspa_ctx* ctx, const double* lifts, int B) {
  ProfScope ps(ctx, LSSPA_K_PAIRS);
  const int d = ctx->pairs_d;
  HIPCHK(launch_pairs(lifts, d, ctx->pr_perms.ptr, d, B, ctx->pr_delta.ptr, ctx->pr_pos.ptr, ctx->pr_count.ptr,
                      ctx->pr_mean.ptr, ctx->pr_m2.ptr, ctx->pr_phi.ptr, ctx->stream));
  ctx->pairs_n += B;
  return LSSPA_OK;
}

}  // namespace

int lsspa_pairs_enable(lsspa_ctx* ctx, int32_t on) try {
  if (!ctx) return LSSPA_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  if (!on) {
    TRY(sync_all(ctx));
    ctx->pairs_on = false;
    dev_free(ctx->pr_count); dev_free(ctx->pr_mean); dev_free(ctx->pr_m2); dev_free(ctx->pr_phi);
    dev_free(ctx->pr_delta); dev_free(ctx->pr_lifts); dev_free(ctx->pr_pos); dev_free(ctx->pr_perms);
    return LSSPA_OK;
  }
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  const int d = ctx->sd();
  if (d < 2 || d > LSSPA_PAIRS_MAX_D) {
    char msg[200];
    snprintf(msg, sizeof msg, "sampled pairwise interactions take 2 <= d <= LSSPA_PAIRS_MAX_D = %d players (16-bit "
             "positions, three d x d tables); this problem has d = %d", LSSPA_PAIRS_MAX_D, d);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  TRY(sync_all(ctx));
  ctx->pairs_on = false;
  const size_t dd = (size_t)d * d;
  TRY(dev_alloc(ctx, ctx->pr_count, dd));
  TRY(dev_alloc(ctx, ctx->pr_mean, dd));
  TRY(dev_alloc(ctx, ctx->pr_m2, dd));
  TRY(dev_alloc(ctx, ctx->pr_phi, (size_t)d));
  ctx->pairs_d = d;
  TRY(pairs_zero(ctx));
  ctx->pairs_on = true;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_pairs_reset(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(pairs_usable(ctx));
  HIPCHK(hipSetDevice(ctx->device));
  return pairs_zero(ctx);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_pairs_batch(lsspa_ctx* ctx, const int32_t* perms, int32_t B) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(pairs_usable(ctx));
  if (!perms || B < 1 || B > (1 << 20)) return ctx->fail(LSSPA_ERR_ARG, "perms / B");
  for (const Lane& L : ctx->lanes)
    if (L.in_flight) return ctx->fail(LSSPA_ERR_STATE, "a launched batch is still to be collected");
  HIPCHK(hipSetDevice(ctx->device));
  const int d = ctx->pairs_d;
  if (!all_permutations(perms, B, d, ctx->perm_mark))
    return ctx->fail(LSSPA_ERR_ARG, ctx->g_players ? "perms: a row is not a permutation of the groups 0..g-1"
                                                   : "perms: a row is not a permutation of 0..p-1");
  ctx->pr_rows.resize((size_t)3 * B * d);
  expand_pair_rows(perms, B, d, ctx->pr_rows.data());
  TRY(pairs_stage(ctx, perms, B));
  Lane* L = nullptr;
  TRY(lift_launch(ctx, ctx->pr_rows.data(), 3 * B, 1, &L));   // unpaired: three rows a sample
  // from here on the lane is this call's to give back, whatever happens
  int rc = LSSPA_OK;
  if (ctx->n_lanes == 2 && hipStreamWaitEvent(ctx->stream, L->ev_done, 0) != hipSuccess)
    rc = ctx->fail(LSSPA_ERR_HIP, "hipStreamWaitEvent");
  if (rc == LSSPA_OK) rc = pairs_kernels(ctx, lane_out(ctx, *L), B);
  const int rc2 = lane_taken(ctx, *L, L->B);
  L->in_flight = false;
  return rc != LSSPA_OK ? rc : rc2;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_pairs_get(lsspa_ctx* ctx, int64_t* n_samples, double* phi, int64_t* count, double* mean, double* m2) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(pairs_usable(ctx));
  HIPCHK(hipSetDevice(ctx->device));
  TRY(sync_all(ctx));
  const size_t d = (size_t)ctx->pairs_d, dd = d * d;
  if (n_samples) *n_samples = ctx->pairs_n;
  if (phi) {
    HIPCHK(hipMemcpy(phi, ctx->pr_phi.ptr, d * 8, hipMemcpyDeviceToHost));
    const double scale = ctx->pairs_n > 0 ? 1.0 / (3.0 * (double)ctx->pairs_n) : 0.0;
    for (size_t j = 0; j < d; ++j) phi[j] *= scale;
  }
  // the device keeps a pair at [a][b], a < b (the rest of its tables stays zero): mirrored here
  auto mirror = [d](auto* t) {
    for (size_t a = 0; a < d; ++a) {
      t[a * d + a] = 0;
      for (size_t b = a + 1; b < d; ++b) t[b * d + a] = t[a * d + b];
    }
  };
  if (count) {
    HIPCHK(hipMemcpy(count, ctx->pr_count.ptr, dd * sizeof(int64_t), hipMemcpyDeviceToHost));
    mirror(count);
  }
  if (mean) {
    HIPCHK(hipMemcpy(mean, ctx->pr_mean.ptr, dd * 8, hipMemcpyDeviceToHost));
    mirror(mean);
  }
  if (m2) {
    HIPCHK(hipMemcpy(m2, ctx->pr_m2.ptr, dd * 8, hipMemcpyDeviceToHost));
    mirror(m2);
  }
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_expand_pairs(int32_t d, const int32_t* perms, int32_t B, int32_t* out) try {
  if (!perms || !out || d < 1 || B < 1) return LSSPA_ERR_ARG;
  std::vector<int32_t> mark;
  if (!all_permutations(perms, B, d, mark)) return LSSPA_ERR_ARG;
  expand_pair_rows(perms, B, d, out);
  return LSSPA_OK;
} catch (...) {
  return abi_caught(nullptr);
}

int lsspa_debug_pairs_inject(lsspa_ctx* ctx, const double* lifts, const int32_t* perms, int32_t B) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(pairs_usable(ctx));
  if (!lifts || !perms || B < 1 || B > (1 << 20)) return ctx->fail(LSSPA_ERR_ARG, "lifts / perms / B");
  HIPCHK(hipSetDevice(ctx->device));
  const int d = ctx->pairs_d;
  if (!all_permutations(perms, B, d, ctx->perm_mark))
    return ctx->fail(LSSPA_ERR_ARG, "perms: a row is not a permutation of 0..d-1");
  const size_t cnt = (size_t)3 * B * d;
  if (ctx->pr_lifts.count < cnt) HIPCHK(hipStreamSynchronize(ctx->stream));
  TRY(dev_alloc(ctx, ctx->pr_lifts, cnt));
  TRY(pairs_stage(ctx, perms, B));
  HIPCHK(hipMemcpyAsync(ctx->pr_lifts.ptr, lifts, cnt * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));   // lifts is the caller's (pageable, possibly temporary) buffer
  TRY(pairs_kernels(ctx, ctx->pr_lifts.ptr, B));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_get_info(lsspa_ctx* ctx, int32_t* info) try {
  if (!ctx || !info) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  HIPCHK(hipSetDevice(ctx->device));
  TRY(sync_all(ctx));   // the flag is raised by kernels on the lanes' streams
  HIPCHK(hipMemcpyAsync(info, ctx->info_d.ptr, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_get_sum_deviation(lsspa_ctx* ctx, double* max_deviation) try {
  if (!ctx || !max_deviation) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  HIPCHK(hipSetDevice(ctx->device));
  TRY(sync_all(ctx));
  HIPCHK(hipMemcpyAsync(max_deviation, ctx->info_d.ptr + 2, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_get_info_collected(lsspa_ctx* ctx, int32_t* info) try {
  if (!ctx || !info) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  HIPCHK(hipSetDevice(ctx->device));
  // the context's stream is ordered behind every batch that was collected (lift_collect waits for the lane's last
  // kernel before the statistics read its lift vectors): the bits of those batches are in place when it has drained
  HIPCHK(hipMemcpyAsync(info, ctx->info_d.ptr, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_stats_reset(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  HIPCHK(hipSetDevice(ctx->device));
  return stats_reset(ctx);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_stats_pending(lsspa_ctx* ctx, void** device_ptr, int64_t* count) try {
  if (!ctx || !device_ptr || !count) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  *device_ptr = ctx->pend.ptr;
  *count = (int64_t)1 + ctx->sd() + (int64_t)ctx->sd() * ctx->sd();
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_stats_merge(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  HIPCHK(hipSetDevice(ctx->device));
  bool cleared = false;
  {
    ProfScope ps(ctx, LSSPA_K_STATS);
    HIPCHK(launch_stats_merge(ctx->pend.ptr, ctx->state_n.ptr, ctx->mean.ptr, ctx->M2.ptr, ctx->sd(), ctx->stream,
                              &cleared));
  }
  // an empty pending buffer (n_b = 0) is what a rank with no samples contributes
  if (!cleared)
    HIPCHK(hipMemsetAsync(ctx->pend.ptr, 0, sizeof(double) * ((size_t)1 + ctx->p + (size_t)ctx->p * ctx->p),
                          ctx->stream));
  ctx->pend_dirty = false;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_stats_get(lsspa_ctx* ctx, int64_t* n, double* mean, double* cov_biased) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  HIPCHK(hipSetDevice(ctx->device));
  const size_t p = ctx->sd();
  double nd = 0.0;
  HIPCHK(hipMemcpyAsync(&nd, ctx->state_n.ptr, 8, hipMemcpyDeviceToHost, ctx->stream));
  if (mean) HIPCHK(hipMemcpyAsync(mean, ctx->mean.ptr, p * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (cov_biased) HIPCHK(hipMemcpyAsync(cov_biased, ctx->M2.ptr, p * p * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (n) *n = (int64_t)llround(nd);
  if (cov_biased && nd > 0.0) {
    const double inv = 1.0 / nd;
    for (size_t i = 0; i < p * p; ++i) cov_biased[i] *= inv;
  }
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_stats_set(lsspa_ctx* ctx, int64_t n, const double* mean, const double* cov_biased) try {
  if (!ctx || !mean || !cov_biased || n < 0) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  HIPCHK(hipSetDevice(ctx->device));
  const size_t p = ctx->sd();
  std::vector<double> m2(p * p);
  for (size_t i = 0; i < p * p; ++i) m2[i] = cov_biased[i] * (double)n;
  double st[8] = {(double)n, 0, 0, 0, 0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(ctx->state_n.ptr, st, sizeof st, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->mean.ptr, mean, p * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->M2.ptr, m2.data(), p * p * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->pend.ptr, 0, sizeof(double) * ((size_t)1 + p + p * p), ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));   // m2 / st are stack and heap temporaries
  ctx->pend_dirty = false;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

// ---------------------------------------------------------------------------------------------
int lsspa_history_enable(lsspa_ctx* ctx, int64_t capacity) try {
  if (!ctx || capacity < 0) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->hist_n = 0;
  ctx->hist_cap = 0;
  ctx->run_on = false;
  if (capacity == 0) {
    // switched off; small buffers stay (a kept engine's next call of the same shape finds them in place -- three hipFree
    // calls, each a device synchronisation, were 1.2 ms of a 46 ms call); a long history is given back
    if (ctx->hist.count * sizeof(double) > ((size_t)64 << 20)) dev_free(ctx->hist);
    return LSSPA_OK;
  }
  const int64_t rows = ((capacity + KCH - 1) / KCH) * KCH;   // the draws kernel reads whole 16-row chunks
  TRY(dev_alloc(ctx, ctx->hist, (size_t)rows * ctx->ldh()));
  // zero once: padding columns and the rows of a partial last chunk are read (times a zero of Xi)
  HIPCHK(hipMemsetAsync(ctx->hist.ptr, 0, ctx->hist.count * 8, ctx->stream));
  TRY(dev_alloc(ctx, ctx->draws, (size_t)ERR_DRAWS * ctx->ldh()));
  TRY(dev_alloc(ctx, ctx->err_out, 2 * (size_t)ctx->p + 2 + ERR_DRAWS));   // [quantiles, mean, n], row norms
  HIPCHK(hipMemsetAsync(ctx->draws.ptr, 0, ctx->draws.count * 8, ctx->stream));
  ctx->hist_cap = capacity;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_history_get(lsspa_ctx* ctx, int64_t* count, double* lifts) try {
  if (!ctx || !count) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  *count = ctx->hist_n;
  if (lifts && ctx->hist_n > 0) {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpy2DAsync(lifts, (size_t)ctx->sd() * 8, ctx->hist.ptr, (size_t)ctx->ldh() * 8, (size_t)ctx->sd() * 8,
                            (size_t)ctx->hist_n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_history_append(lsspa_ctx* ctx, const double* lifts, int64_t rows) try {
  if (!ctx || rows < 0 || (rows > 0 && !lifts)) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  if (ctx->hist_cap == 0) return ctx->fail(LSSPA_ERR_STATE, "history is not enabled");
  if (rows == 0) return LSSPA_OK;
  HIPCHK(hipSetDevice(ctx->device));
  TRY(hist_append(ctx, lifts, rows, hipMemcpyHostToDevice));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_error_draws(lsspa_ctx* ctx, const double* xi, int64_t ld_xi, int64_t n_local, int64_t n_total) try {
  if (!ctx || n_local < 0 || n_total < n_local || (n_local > 0 && (!xi || ld_xi < n_local)))
    return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  if (ctx->hist_cap == 0) return ctx->fail(LSSPA_ERR_STATE, "history is not enabled");
  if (n_local != ctx->hist_n)
    return ctx->fail(LSSPA_ERR_ARG, "n_local must equal the number of lift vectors in this context's history");
  if (ctx->pend_dirty) return ctx->fail(LSSPA_ERR_STATE, "merge the pending batch first: the mean is stale");
  HIPCHK(hipSetDevice(ctx->device));
  const int ldh = ctx->ldh();
  if (n_local == 0) {   // a rank without samples contributes zeros to the all-reduce
    HIPCHK(hipMemsetAsync(ctx->draws.ptr, 0, ctx->draws.count * 8, ctx->stream));
    return LSSPA_OK;
  }
  const int64_t n_pad = ((n_local + KCH - 1) / KCH) * KCH;
  TRY(dev_alloc(ctx, ctx->xi_d, (size_t)ERR_DRAWS * n_pad));
  if (n_pad != n_local) HIPCHK(hipMemsetAsync(ctx->xi_d.ptr, 0, (size_t)ERR_DRAWS * n_pad * 8, ctx->stream));
  HIPCHK(hipMemcpy2DAsync(ctx->xi_d.ptr, (size_t)n_pad * 8, xi, (size_t)ld_xi * 8, (size_t)n_local * 8, ERR_DRAWS,
                          hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));   // xi is the caller's (pageable, possibly temporary) buffer: it may
                                               // be released as soon as this call returns (lsspa.h)
  const double nt = (double)n_total;
  const double scale = 1.0 / sqrt(nt * (nt - 1.0));   // inf for n_total = 1, as numpy's division gives
  ProfScope ps(ctx, LSSPA_K_ERROR);
  HIPCHK(launch_error_draws(ctx->xi_d.ptr, (int)n_pad, ctx->hist.ptr, ldh, (int)n_pad, ctx->mean.ptr, scale,
                            ctx->sd(), ctx->draws.ptr, ldh, ctx->stream));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_error_buffer(lsspa_ctx* ctx, void** device_ptr, int64_t* count) try {
  if (!ctx || !device_ptr || !count) return LSSPA_ERR_ARG;
  if (ctx->hist_cap == 0) return ctx->fail(LSSPA_ERR_STATE, "history is not enabled");
  *device_ptr = ctx->draws.ptr;
  *count = (int64_t)ERR_DRAWS * ctx->ldh();
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_error_quantiles(lsspa_ctx* ctx, double* feature_errors, double* overall_error) try {
  if (!ctx || !feature_errors || !overall_error) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  if (ctx->hist_cap == 0) return ctx->fail(LSSPA_ERR_STATE, "history is not enabled");
  HIPCHK(hipSetDevice(ctx->device));
  const int p = ctx->sd();
  {
    ProfScope ps(ctx, LSSPA_K_ERROR);
    HIPCHK(launch_error_quantiles(ctx->draws.ptr, ctx->ldh(), p, ctx->err_out.ptr + 2 * p + 2, ctx->err_out.ptr,
                                  ctx->stream));
  }
  std::vector<double> out((size_t)p + 1);
  HIPCHK(hipMemcpyAsync(out.data(), ctx->err_out.ptr, ((size_t)p + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  std::copy(out.begin(), out.begin() + p, feature_errors);
  *overall_error = out[p];
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

// ---- running form of the device-side estimator -------------------------------------------------------------
int lsspa_error_running_enable(lsspa_ctx* ctx, uint64_t seed) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  // the staging of the lift vectors is the history buffer (one chunk at a time; it grows on demand)
  TRY(lsspa_history_enable(ctx, 256));
  const size_t ldh = ctx->ldh();
  TRY(dev_alloc(ctx, ctx->Dacc, (size_t)ERR_DRAWS * ldh));
  TRY(dev_alloc(ctx, ctx->sacc, (size_t)ERR_DRAWS));
  HIPCHK(hipMemsetAsync(ctx->Dacc.ptr, 0, ctx->Dacc.count * 8, ctx->stream));
  HIPCHK(hipMemsetAsync(ctx->sacc.ptr, 0, ctx->sacc.count * 8, ctx->stream));
  const size_t need = (size_t)lsspa_ctx::RES_SLOTS * (2 * (size_t)ctx->p + 2);
  if (ctx->res_h_count < need) {
    if (ctx->res_h) (void)hipHostFree(ctx->res_h);
    ctx->res_h = nullptr;
    ctx->res_h_count = 0;
    if (hipHostMalloc(reinterpret_cast<void**>(&ctx->res_h), need * 8, hipHostMallocMapped | hipHostMallocCoherent) !=
            hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->res_hd), ctx->res_h, 0) != hipSuccess) {
      if (ctx->res_h) (void)hipHostFree(ctx->res_h);
      ctx->res_h = ctx->res_hd = nullptr;
      (void)hipGetLastError();
      return ctx->fail(LSSPA_ERR_NOMEM, "hipHostMalloc (result slots of the estimator)");
    }
    ctx->res_h_count = need;
  }
  for (int k = 0; k < lsspa_ctx::RES_SLOTS; ++k) {
    // (release to system scope: the kernel's stores to the pinned slot are the host's to read once the event is done)
    if (!ctx->res_ev[k])
      HIPCHK(hipEventCreateWithFlags(&ctx->res_ev[k], hipEventDisableTiming | hipEventReleaseToSystem));
    ctx->res_valid[k] = false;
  }
  ctx->run_seed = seed;
  ctx->run_on = true;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_error_advance(lsspa_ctx* ctx, int64_t first_id, int64_t stride) try {
  if (!ctx || first_id < 0 || stride < 1) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  if (!ctx->run_on) return ctx->fail(LSSPA_ERR_STATE, "the running estimator is not enabled");
  const int64_t cnt = ctx->hist_n;
  if (cnt == 0) return LSSPA_OK;
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t n_pad = ((cnt + KCH - 1) / KCH) * KCH;
  TRY(dev_alloc(ctx, ctx->xi_d, (size_t)ERR_DRAWS * n_pad));
  ProfScope ps(ctx, LSSPA_K_ERROR);
  // rows cnt .. n_pad of the staging hold older chunks' (finite) lift vectors: they meet the zero columns of Xi
  HIPCHK(launch_error_accumulate(ctx->run_seed, first_id, stride, (int)cnt, (int)n_pad, ctx->xi_d.ptr, ctx->hist.ptr,
                                 ctx->ldh(), 0, ctx->ldh(), ctx->sd(), ctx->Dacc.ptr, ctx->sacc.ptr, ctx->stream));
  ctx->hist_n = 0;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_error_running_draws(lsspa_ctx* ctx, int64_t n_total) try {
  if (!ctx || n_total < 0) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  if (!ctx->run_on) return ctx->fail(LSSPA_ERR_STATE, "the running estimator is not enabled");
  if (ctx->hist_n != 0) return ctx->fail(LSSPA_ERR_STATE, "collected samples not yet folded in: call lsspa_error_advance");
  if (ctx->pend_dirty) return ctx->fail(LSSPA_ERR_STATE, "merge the pending batch first: the mean is stale");
  HIPCHK(hipSetDevice(ctx->device));
  const double nt = (double)n_total;
  const double scale = 1.0 / sqrt(nt * (nt - 1.0));   // inf for n_total = 1, as numpy's division gives
  ProfScope ps(ctx, LSSPA_K_ERROR);
  HIPCHK(launch_error_running_draws(ctx->Dacc.ptr, ctx->sacc.ptr, ctx->mean.ptr, scale, ctx->sd(), ctx->ldh(),
                                    ctx->draws.ptr, ctx->stream));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

// the shared tail of the two enqueue forms: the quantile kernel has written [quantiles, mean, n] into the pinned slot
// itself; its event tells the host when
// record == false (lsspa_group_collect, all but the group's last check): the slot shares the event of a LATER check of
// the same call -- a host that reads its checks group by group need not pay an event per check
static int finish_check(lsspa_ctx* ctx, int slot, bool record = true) {
  if (record) HIPCHK(hipEventRecord(ctx->res_ev[slot], ctx->stream));
  ctx->res_valid[slot] = true;
  ctx->res_via[slot] = slot;
  return LSSPA_OK;
}

static int quantiles_enqueue(lsspa_ctx* ctx, int32_t slot, bool record);
int lsspa_error_quantiles_enqueue(lsspa_ctx* ctx, int32_t slot) try {
  return quantiles_enqueue(ctx, slot, true);
} catch (...) {
  return abi_caught(ctx);
}

static int quantiles_enqueue(lsspa_ctx* ctx, int32_t slot, bool record) {
  if (!ctx || slot < 0 || slot >= lsspa_ctx::RES_SLOTS) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  if (!ctx->run_on) return ctx->fail(LSSPA_ERR_STATE, "the running estimator is not enabled");
  HIPCHK(hipSetDevice(ctx->device));
  const size_t p = ctx->sd();
  {
    ProfScope ps(ctx, LSSPA_K_ERROR);
    HIPCHK(launch_error_quantiles(ctx->draws.ptr, ctx->ldh(), (int)p, ctx->err_out.ptr + 2 * p + 2,
                                  ctx->res_hd + (size_t)slot * (2 * p + 2), ctx->stream, ctx->mean.ptr,
                                  ctx->state_n.ptr));
  }
  return finish_check(ctx, slot, record);
}

static int check_enqueue(lsspa_ctx* ctx, int64_t n_total, int32_t slot, bool record);
int lsspa_error_check_enqueue(lsspa_ctx* ctx, int64_t n_total, int32_t slot) try {
  return check_enqueue(ctx, n_total, slot, true);
} catch (...) {
  return abi_caught(ctx);
}

static int check_enqueue(lsspa_ctx* ctx, int64_t n_total, int32_t slot, bool record) {
  if (!ctx || n_total < 0 || slot < 0 || slot >= lsspa_ctx::RES_SLOTS) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  if (!ctx->run_on) return ctx->fail(LSSPA_ERR_STATE, "the running estimator is not enabled");
  if (ctx->hist_n != 0) return ctx->fail(LSSPA_ERR_STATE, "collected samples not yet folded in: call lsspa_error_advance");
  if (ctx->pend_dirty) return ctx->fail(LSSPA_ERR_STATE, "merge the pending batch first: the mean is stale");
  HIPCHK(hipSetDevice(ctx->device));
  const size_t p = ctx->sd();
  const double nt = (double)n_total;
  const double scale = 1.0 / sqrt(nt * (nt - 1.0));
  {
    ProfScope ps(ctx, LSSPA_K_ERROR);
    HIPCHK(launch_error_quantiles_running(ctx->Dacc.ptr, ctx->sacc.ptr, ctx->mean.ptr, scale, ctx->ldh(), (int)p,
                                          ctx->err_out.ptr + 2 * p + 2, ctx->res_hd + (size_t)slot * (2 * p + 2),
                                          ctx->state_n.ptr, ctx->stream));
  }
  return finish_check(ctx, slot, record);
}

int lsspa_error_result(lsspa_ctx* ctx, int32_t slot, int32_t wait, int32_t* ready, double* feature_errors,
                       double* overall_error, double* mean, int64_t* n) try {
  if (!ctx || slot < 0 || slot >= lsspa_ctx::RES_SLOTS || !ready) return LSSPA_ERR_ARG;
  if (!ctx->run_on || !ctx->res_valid[slot]) return ctx->fail(LSSPA_ERR_STATE, "nothing was enqueued into this slot");
  HIPCHK(hipSetDevice(ctx->device));
  const int via = ctx->res_via[slot];
  if (wait) {
    HIPCHK(hipEventSynchronize(ctx->res_ev[via]));
  } else {
    const hipError_t e = hipEventQuery(ctx->res_ev[via]);
    if (e == hipErrorNotReady) {
      (void)hipGetLastError();
      *ready = 0;
      return LSSPA_OK;
    }
    HIPCHK(e);
  }
  const size_t p = ctx->sd();
  const double* src = ctx->res_h + (size_t)slot * (2 * p + 2);
  if (feature_errors) std::copy(src, src + p, feature_errors);
  if (overall_error) *overall_error = src[p];
  if (mean) std::copy(src + p + 1, src + 2 * p + 1, mean);
  if (n) *n = (int64_t)llround(src[2 * p + 1]);
  *ready = 1;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_error_state_get(lsspa_ctx* ctx, double* D, double* s) try {
  if (!ctx || !D || !s) return LSSPA_ERR_ARG;
  if (!ctx->run_on) return ctx->fail(LSSPA_ERR_STATE, "the running estimator is not enabled");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpy2DAsync(D, (size_t)ctx->sd() * 8, ctx->Dacc.ptr, (size_t)ctx->ldh() * 8, (size_t)ctx->sd() * 8, ERR_DRAWS,
                          hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(s, ctx->sacc.ptr, (size_t)ERR_DRAWS * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_error_state_set(lsspa_ctx* ctx, const double* D, const double* s) try {
  if (!ctx || !D || !s) return LSSPA_ERR_ARG;
  if (!ctx->run_on) return ctx->fail(LSSPA_ERR_STATE, "the running estimator is not enabled");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpy2DAsync(ctx->Dacc.ptr, (size_t)ctx->ldh() * 8, D, (size_t)ctx->sd() * 8, (size_t)ctx->sd() * 8, ERR_DRAWS,
                          hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->sacc.ptr, s, (size_t)ERR_DRAWS * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_error_xi(lsspa_ctx* ctx, uint64_t seed, int64_t first_id, int64_t stride, int64_t count, double* xi) try {
  if (!ctx || !xi || count < 1 || count > (1 << 20) || first_id < 0 || stride < 1) return LSSPA_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t n_pad = ((count + KCH - 1) / KCH) * KCH;
  TRY(dev_alloc(ctx, ctx->xi_d, (size_t)ERR_DRAWS * n_pad));
  HIPCHK(launch_error_xi(seed, first_id, stride, (int)count, (int)n_pad, ctx->xi_d.ptr, ctx->stream));
  HIPCHK(hipMemcpy2DAsync(xi, (size_t)count * 8, ctx->xi_d.ptr, (size_t)n_pad * 8, (size_t)count * 8, ERR_DRAWS,
                          hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

// The per-chunk tail of a launched group in ONE call (the host loop of a small problem is bound by its own call
// overhead otherwise: a chunk of 256 orderings takes the GPU 37 us at p = 100).  For every chunk c, in order:
// collect (fold into the statistics), all-reduce + merge when the context's communicator spans several ranks, fold the
// chunk into the running estimator, and -- where n_after[c] > 0 -- enqueue the check of that sample count into slot[c].
int lsspa_group_collect(lsspa_ctx* ctx, int32_t ticket, int32_t n_chunks, const int32_t* first, const int32_t* count,
                        const int64_t* first_id, int64_t stride, const int64_t* n_after, const int32_t* slot) try {
  if (!ctx || ticket < 0 || ticket > 1 || n_chunks < 1 || !first || !count || !first_id || !n_after || !slot)
    return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  if (!ctx->run_on) return ctx->fail(LSSPA_ERR_STATE, "the running estimator is not enabled");
  if (ctx->hist_n != 0) return ctx->fail(LSSPA_ERR_STATE, "collected samples not yet folded in: call lsspa_error_advance");
  if (stride < 1) return ctx->fail(LSSPA_ERR_ARG, "stride must be positive");
  for (int c = 0; c < n_chunks; ++c)
    if (first_id[c] < 0 || n_after[c] < 0 || slot[c] < 0 || slot[c] >= lsspa_ctx::RES_SLOTS)
      return ctx->fail(LSSPA_ERR_ARG, "sample ids and counts must be non-negative, slots within range");
  HIPCHK(hipSetDevice(ctx->device));
  {   // the chunks follow each other from the lane's next sample on, inside the batch: checked before the first is taken
    const Lane& Lc = ctx->lanes[ticket];
    if (!Lc.in_flight) return ctx->fail(LSSPA_ERR_STATE, "no launched batch on this lane");
    int64_t next = Lc.taken;
    for (int c = 0; c < n_chunks; ++c) {
      if (count[c] < 0 || (count[c] > 0 && first[c] != next))
        return ctx->fail(LSSPA_ERR_ARG, "parts of a launched batch are collected front to back, without gaps");
      next += count[c];
    }
    if (next > Lc.B) return ctx->fail(LSSPA_ERR_ARG, "the chunks reach beyond the launched batch");
  }
  // a communicator on the context (of one rank or of many): the moments and the draws go through it, as in the
  // separate calls; none: the chunk is folded and merged at once
  const bool several = ctx->comm != nullptr;
  int last_check = -1;
  for (int c = 0; c < n_chunks; ++c)
    if (n_after[c] > 0) last_check = c;
  Lane& Lg = ctx->lanes[ticket];
  if (chunks_fusable(ctx, Lg, n_chunks, first, count)) {
    // small problem, one rank: the group's statistics in one launch; every check reads the mean and n after ITS chunk
    // ... and the estimator likewise: the chunks' products side by side, summed in order with a snapshot per chunk, all
    // the checks' quantiles in one launch (launch_error_group) -- five launches a group instead of five a chunk
    EstChunks ch;
    EstChecks ck;
    ch.n = n_chunks;
    ck.n = 0;
    long long off = 0;
    for (int c = 0; c < n_chunks; ++c) {
      ch.first[c] = first[c];
      ch.count[c] = count[c];
      ch.n_pad[c] = ((count[c] + KCH - 1) / KCH) * KCH;
      ch.xi_off[c] = off;
      off += (long long)ERR_DRAWS * ch.n_pad[c];
      ch.first_id[c] = first_id[c];
      ch.scale[c] = 0.0;
      if (n_after[c] > 0) {
        const double nt = (double)n_after[c];
        ch.scale[c] = 1.0 / sqrt(nt * (nt - 1.0));
        ck.chunk[ck.n] = c;
        ck.slot[ck.n] = slot[c];
        ck.scale[ck.n] = ch.scale[c];
        ++ck.n;
      }
    }
    const size_t ld = ctx->ldh();
    TRY(dev_alloc(ctx, ctx->xi_d, (size_t)off));
    TRY(dev_alloc(ctx, ctx->grp_P, (size_t)n_chunks * ERR_DRAWS * ld));
    TRY(dev_alloc(ctx, ctx->grp_D, (size_t)n_chunks * ERR_DRAWS * ld));
    TRY(dev_alloc(ctx, ctx->grp_S, (size_t)n_chunks * ERR_DRAWS));
    TRY(dev_alloc(ctx, ctx->grp_s, (size_t)n_chunks * ERR_DRAWS));
    TRY(dev_alloc(ctx, ctx->grp_norms, (size_t)n_chunks * ERR_DRAWS));
    // (every buffer is there before the first launch: a refused allocation leaves statistics and estimator in step)
    TRY(collect_chunks_small(ctx, Lg, n_chunks, first, count, true));
    {
      ProfScope ps(ctx, LSSPA_K_ERROR);
      HIPCHK(launch_error_group(ctx->run_seed, stride, ch, ck, ctx->xi_d.ptr, lane_out(ctx, Lg), ctx->sd(), (int)ld,
                                ctx->grp_P.ptr, ctx->grp_S.ptr, ctx->Dacc.ptr, ctx->sacc.ptr, ctx->grp_D.ptr,
                                ctx->grp_s.ptr, ctx->mean_snap.ptr, ctx->n_snap.ptr, ctx->grp_norms.ptr, ctx->res_hd,
                                ctx->stream));
    }
    for (int c = 0; c < n_chunks; ++c)
      if (n_after[c] > 0) TRY(finish_check(ctx, slot[c], c == last_check));
    TRY(lane_taken(ctx, Lg, first[n_chunks - 1] + count[n_chunks - 1]));
    for (int c = 0; c < n_chunks; ++c)
      if (n_after[c] > 0) ctx->res_via[slot[c]] = slot[last_check];
    return LSSPA_OK;
  }
  for (int c = 0; c < n_chunks; ++c) {
    if (count[c] > 0) {
      const int64_t ids[2] = {first_id[c], stride};
      TRY(lift_collect(ctx, ctx->lanes[ticket], first[c], count[c], nullptr, several ? 1 : 2, ids));
    }
    if (several) {
      TRY(lsspa_stats_allreduce(ctx));
      TRY(lsspa_stats_merge(ctx));
    }
    if (n_after[c] > 0) {
      const bool record = (c == last_check);
      if (several) {
        TRY(lsspa_error_running_draws(ctx, n_after[c]));
        TRY(lsspa_error_allreduce(ctx));
        TRY(quantiles_enqueue(ctx, slot[c], record));
      } else {
        TRY(check_enqueue(ctx, n_after[c], slot[c], record));
      }
    }
  }
  // the earlier checks of the call are done when its last one is: they are read through that slot's event
  for (int c = 0; c < n_chunks; ++c)
    if (n_after[c] > 0) ctx->res_via[slot[c]] = slot[last_check];
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

// ---------------------------------------------------------------------------------------------
// Collectives: RCCL on the context's stream, so kernels -> all-reduce -> merge need no host synchronisation.
int lsspa_comm_unique_id(uint8_t* id128) try {
  std::string err;
  if (comm_unique_id(id128, err) != 0) {
    g_create_error = err;
    return LSSPA_ERR_HIP;
  }
  return LSSPA_OK;
} catch (...) {
  return abi_caught(nullptr);
}

int lsspa_comm_init(lsspa_ctx* ctx, const uint8_t* id128, int32_t rank, int32_t world) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!id128 || world < 1 || rank < 0 || rank >= world) return ctx->fail(LSSPA_ERR_ARG, "need an id and 0 <= rank < world");
  if (ctx->comm) return ctx->fail(LSSPA_ERR_STATE, "this context already has a communicator");
  HIPCHK(hipSetDevice(ctx->device));
  std::string err;
  if (comm_create(id128, rank, world, ctx->device, &ctx->comm, err) != 0) return ctx->fail(LSSPA_ERR_HIP, err.c_str());
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_comm_destroy(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!ctx->comm) return LSSPA_OK;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  comm_destroy(ctx->comm);
  ctx->comm = nullptr;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_comm_info(const lsspa_ctx* ctx, int32_t* rank, int32_t* world) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (rank) *rank = comm_rank(ctx->comm);
  if (world) *world = comm_world(ctx->comm);
  return ctx->comm ? LSSPA_OK : LSSPA_ERR_STATE;
} catch (...) {
  return abi_caught(const_cast<lsspa_ctx*>(ctx));
}

static int allreduce_buffer(lsspa_ctx* ctx, double* buf, size_t count) {
  std::string err;
  if (comm_allreduce_f64(ctx->comm, buf, count, ctx->stream, err) != 0) return ctx->fail(LSSPA_ERR_HIP, err.c_str());
  return LSSPA_OK;
}

int lsspa_stats_allreduce(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  if (!ctx->comm) return ctx->fail(LSSPA_ERR_STATE, "no communicator: call lsspa_comm_init first");
  HIPCHK(hipSetDevice(ctx->device));
  const int p = ctx->sd();
  ProfScope ps(ctx, LSSPA_K_COMM);
  if (p < ctx->pack_from_p) return allreduce_buffer(ctx, ctx->pend.ptr, (size_t)1 + p + (size_t)p * p);
  const size_t cnt = (size_t)stats_packed_count(p);
  TRY(dev_alloc(ctx, ctx->pack, cnt));
  HIPCHK(launch_stats_pack(ctx->pend.ptr, ctx->pack.ptr, p, ctx->stream));
  TRY(allreduce_buffer(ctx, ctx->pack.ptr, cnt));
  HIPCHK(launch_stats_unpack(ctx->pack.ptr, ctx->pend.ptr, p, ctx->stream));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_reduce_allreduce(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!ctx->reduce_open) return ctx->fail(LSSPA_ERR_STATE, "no partial reduction in progress");
  if (!ctx->comm) return ctx->fail(LSSPA_ERR_STATE, "no communicator: call lsspa_comm_init first");
  HIPCHK(hipSetDevice(ctx->device));
  const size_t P1pad = (size_t)round_up(ctx->p + 1, 128);
  ProfScope ps(ctx, LSSPA_K_COMM);
  return allreduce_buffer(ctx, ctx->Cred.ptr, 2 * P1pad * P1pad);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_error_allreduce(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (ctx->hist_cap == 0) return ctx->fail(LSSPA_ERR_STATE, "history is not enabled");
  if (!ctx->comm) return ctx->fail(LSSPA_ERR_STATE, "no communicator: call lsspa_comm_init first");
  HIPCHK(hipSetDevice(ctx->device));
  ProfScope ps(ctx, LSSPA_K_COMM);
  return allreduce_buffer(ctx, ctx->draws.ptr, (size_t)ERR_DRAWS * ctx->ldh());
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_comm_sum_i64(lsspa_ctx* ctx, int64_t* values, int32_t count) try {
  if (!ctx || !values || count < 1) return LSSPA_ERR_ARG;
  if (!ctx->comm) return ctx->fail(LSSPA_ERR_STATE, "no communicator: call lsspa_comm_init first");
  HIPCHK(hipSetDevice(ctx->device));
  TRY(dev_alloc(ctx, ctx->ibuf, (size_t)count));
  HIPCHK(hipMemcpyAsync(ctx->ibuf.ptr, values, (size_t)count * 8, hipMemcpyHostToDevice, ctx->stream));
  std::string err;
  if (comm_allreduce_i64(ctx->comm, ctx->ibuf.ptr, (size_t)count, ctx->stream, err) != 0)
    return ctx->fail(LSSPA_ERR_HIP, err.c_str());
  HIPCHK(hipMemcpyAsync(values, ctx->ibuf.ptr, (size_t)count * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_comm_allgather(lsspa_ctx* ctx, const double* send, int64_t count, double* recv) try {
  if (!ctx || count < 0 || (count > 0 && (!send || !recv))) return LSSPA_ERR_ARG;
  if (!ctx->comm) return ctx->fail(LSSPA_ERR_STATE, "no communicator: call lsspa_comm_init first");
  if (count == 0) return LSSPA_OK;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t world = (size_t)comm_world(ctx->comm), cnt = (size_t)count;
  TRY(dev_alloc(ctx, ctx->xfer, (world + 1) * cnt));
  double* d_send = ctx->xfer.ptr;
  double* d_recv = ctx->xfer.ptr + cnt;
  HIPCHK(hipMemcpyAsync(d_send, send, cnt * 8, hipMemcpyHostToDevice, ctx->stream));
  std::string err;
  if (comm_allgather_f64(ctx->comm, d_send, d_recv, cnt, ctx->stream, err) != 0)
    return ctx->fail(LSSPA_ERR_HIP, err.c_str());
  HIPCHK(hipMemcpyAsync(recv, d_recv, world * cnt * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

// ---------------------------------------------------------------------------------------------
int lsspa_profile_enable(lsspa_ctx* ctx, int32_t on) try {
  if (!ctx) return LSSPA_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  TRY(prof_collect(ctx));
  ctx->prof_on = on != 0;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_profile_get(lsspa_ctx* ctx, int32_t k, double* total_ms, int64_t* launches) try {
  if (!ctx || k < 0 || k >= LSSPA_K_COUNT) return LSSPA_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  TRY(prof_collect(ctx));
  if (total_ms) *total_ms = ctx->prof_ms[k];
  if (launches) *launches = ctx->prof_n[k];
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_profile_reset(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  TRY(prof_collect(ctx));
  for (int k = 0; k < LSSPA_K_COUNT; ++k) {
    ctx->prof_ms[k] = 0.0;
    ctx->prof_n[k] = 0;
  }
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

// ---------------------------------------------------------------------------------------------
int lsspa_set_flags(lsspa_ctx* ctx, int32_t flags) try {
  if (!ctx) return LSSPA_ERR_ARG;
  ctx->flags = flags;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_set_r2(lsspa_ctx* ctx, double r2) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!ctx->r2_valid) return ctx->fail(LSSPA_ERR_STATE, "no R^2 yet: call lsspa_full_fit first");
  ctx->r2 = r2;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_host_argsort_rows(const double* keys, int64_t B, int32_t p, int32_t* out, uint8_t* redo, int32_t threads,
                            int64_t* n_redo) try {
  if (!keys || !out || !redo || B < 1 || p < 1 || !n_redo) return LSSPA_ERR_ARG;
  *n_redo = argsort_rows_host(keys, B, p, out, redo, threads);
  return LSSPA_OK;
} catch (...) {
  return abi_caught(nullptr);
}

int lsspa_sampler_create(int32_t p, int32_t bits, const uint64_t* sv, const uint64_t* q0, double scale, int64_t limit,
                         int32_t block, int64_t ahead, int64_t ahead_unasked, int32_t threads, int32_t rank,
                         int32_t world, void** out) try {
  if (!out) return LSSPA_ERR_ARG;
  *out = nullptr;
  if (p < 1 || bits < 1 || bits > 64 || !sv || !q0 || !(scale > 0.0) || limit < 0 || block < 1 || ahead < 1 ||
      ahead_unasked < 1 || threads < 1 || world < 1 || rank < 0 || rank >= world) {
    g_create_error = "lsspa_sampler_create: bad argument";
    return LSSPA_ERR_ARG;
  }
  *out = sobol_sampler_create(p, bits, sv, q0, scale, limit, block, ahead, ahead_unasked, threads, rank, world);
  return LSSPA_OK;
} catch (...) {
  return abi_caught(nullptr);
}

int lsspa_sampler_take(void* sampler, int64_t count, int32_t* out, int64_t cap, int64_t* n_taken, int64_t* n_own,
                       int64_t* redo_pos, int64_t* redo_id, int64_t* n_redo) try {
  if (!sampler || count < 0 || !out || cap < 0 || !n_taken || !n_own || !redo_pos || !redo_id || !n_redo)
    return LSSPA_ERR_ARG;
  const char* err = nullptr;
  const int rc = sobol_sampler_take(static_cast<SobolSampler*>(sampler), count, out, cap, n_taken, n_own, redo_pos,
                                    redo_id, n_redo, &err);
  if (rc == 1) {
    g_create_error = "lsspa_sampler_take: the output buffer is too small for this rank's share";
    return LSSPA_ERR_ARG;
  }
  if (rc == 2) {
    g_create_error = std::string("lsspa_sampler: ") + (err ? err : "the producer failed");
    return LSSPA_ERR_STATE;
  }
  return LSSPA_OK;
} catch (...) {
  return abi_caught(nullptr);
}

int lsspa_sampler_destroy(void* sampler) try {
  sobol_sampler_destroy(static_cast<SobolSampler*>(sampler));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(nullptr);
}

int lsspa_debug_check_perms(const int32_t* perms, int32_t B, int32_t p, int32_t plain) try {
  if (!perms || B < 1 || p < 1) return 0;
  std::vector<int32_t> mark;
  return (plain ? all_permutations_plain(perms, B, p, mark) : all_permutations(perms, B, p, mark)) ? 1 : 0;
} catch (...) {
  return 0;
}

int lsspa_debug_pack_from(lsspa_ctx* ctx, int32_t p_min) try {
  if (!ctx || p_min < 1) return LSSPA_ERR_ARG;
  ctx->pack_from_p = p_min;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_fail_alloc(lsspa_ctx* ctx, int32_t nth) try {
  if (!ctx || nth < 0) return LSSPA_ERR_ARG;
  ctx->fail_alloc_in = nth;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

// Chosen lift vectors in front of the collect paths: a host [B][p] matrix goes into the lane's lift buffer and the lane
// is marked as lift_launch leaves it.  Nothing downstream knows the difference.
int lsspa_debug_lift_inject(lsspa_ctx* ctx, const double* lifts, int32_t B, int32_t* ticket) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!lifts || B < 1 || !ticket) return ctx->fail(LSSPA_ERR_ARG, "lifts / B / ticket");
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  if (ctx->n_lanes != 1) return ctx->fail(LSSPA_ERR_STATE, "lift vectors are injected on a one-lane context only");
  if (ctx->g_players) return ctx->fail(LSSPA_ERR_STATE, "lift vectors are not injected under a player map");
  Lane& L = ctx->lanes[0];
  if (L.in_flight) return ctx->fail(LSSPA_ERR_STATE, "a launched batch is still to be collected");
  HIPCHK(hipSetDevice(ctx->device));
  TRY(ensure_workspace(ctx, L, 0, B));     // the lift buffer alone: no ordering is factored
  HIPCHK(hipMemcpyAsync(L.lifts.ptr, lifts, sizeof(double) * (size_t)B * ctx->p, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));   // lifts is the caller's (pageable, possibly temporary) buffer
  L.B = B;
  L.per = 1;
  L.taken = 0;
  L.in_flight = true;
  ctx->lane_last = 0;
  *ticket = 0;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_stats_slices(int32_t n_samples, int32_t p, int32_t* n_slices, int32_t* per_slice, int32_t* small) try {
  if (n_samples < 1 || p < 1 || !n_slices || !per_slice || !small) return LSSPA_ERR_ARG;
  *small = stats_small_fusable(n_samples, p) ? 1 : 0;
  *n_slices = stats_batch_slices(n_samples, p);
  *per_slice = *n_slices > 1 ? stats_batch_per_slice(n_samples, *n_slices) : n_samples;
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_ARG;
}

int lsspa_debug_gram_plan(int64_t n, int32_t p, int32_t* n_split, int32_t* cnt3, int32_t* slices3, int32_t* rps3,
                          int32_t* nt, int32_t* xlive) try {
  if (n < 1 || p < 1 || !n_split || !cnt3 || !slices3 || !rps3 || !nt || !xlive) return LSSPA_ERR_ARG;
  *n_split = gram_default_split(n, p);
  const GramPlan g = gram_plan(n, p, *n_split);
  for (int c = 0; c < 3; ++c) {
    cnt3[c] = g.cnt[c];
    slices3[c] = g.slices[c];
    rps3[c] = g.rps[c];
  }
  *nt = g.nt;
  *xlive = g.xlive;
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_ARG;
}

static void panel_plan_out(int Jo, const PanelPlan& pp, int32_t* o) {
  o[0] = Jo;
  o[1] = pp.n_lt;
  o[2] = pp.n_x;
  o[3] = pp.grouped;
  o[4] = pp.xlast;
  o[5] = (int32_t)pp.grid;      // panel_plan refuses a grid beyond 2^31 - 1
  o[6] = pp.p_live;
  o[7] = pp.n_ord;
}

int lsspa_debug_panel_plan(int32_t p, int32_t n_ord, int32_t tri, int32_t flags, int32_t* p_pad, int32_t* n_mats,
                           int32_t* n_launch, int32_t* plans, int32_t cap) try {
  if (p < 1 || p > max_features() || n_ord < 1 || n_ord > 0x3fffffff || !p_pad || !n_mats || !n_launch || cap < 0 ||
      (cap > 0 && !plans))
    return LSSPA_ERR_ARG;
  const bool vt = vt_rule(tri, flags);
  *p_pad = work_p_pad(p);
  *n_mats = (tri ? 2 : 1) * n_ord;
  *n_launch = panel_launches(*p_pad, vt);
  for (int Jo = 0; Jo < *n_launch && Jo < cap; ++Jo) {
    PanelPlan pp;
    if (!panel_plan(*p_pad, Jo, *n_mats, n_ord, vt, work_p_live(p), &pp)) return LSSPA_ERR_ARG;
    panel_plan_out(Jo, pp, plans + 8 * Jo);
  }
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_ARG;
}

int lsspa_debug_panel_plan_launch(int32_t p_pad, int32_t Jo, int32_t n_mats, int32_t n_ord, int32_t has_X,
                                  int32_t p_live, int32_t* plan) try {
  PanelPlan pp;
  if (!plan || !panel_plan(p_pad, Jo, n_mats, n_ord, has_X != 0, p_live, &pp)) return LSSPA_ERR_ARG;
  panel_plan_out(Jo, pp, plan);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_ARG;
}

int lsspa_debug_reduce_chunk_rows(lsspa_ctx* ctx, int64_t rows) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (rows != 0 && (rows < 16 || rows % 16 != 0))
    return ctx->fail(LSSPA_ERR_ARG, "rows per streamed chunk: 0 (default) or a multiple of 16");
  ctx->red_chunk_rows = rows;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_set_precision(lsspa_ctx* ctx, int32_t dtype) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (dtype != LSSPA_F64 && dtype != LSSPA_F32) return ctx->fail(LSSPA_ERR_ARG, "dtype");
  HIPCHK(hipSetDevice(ctx->device));
  if ((dtype == LSSPA_F32) != (ctx->f32 != 0)) {
    for (const Lane& L : ctx->lanes)
      if (L.in_flight) return ctx->fail(LSSPA_ERR_STATE, "a launched batch is still to be collected");
    TRY(sync_all(ctx));     // kernels on the lanes' streams still use the workspace that is about to go
    ctx->f32 = dtype == LSSPA_F32;
    free_workspace(ctx);   // re-created for the new element size on demand
  }
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_mfma_probe(lsspa_ctx* ctx, const double* A16x4, const double* B4x16, double* D16x16, int32_t dtype) try {
  if (!ctx || !A16x4 || !B4x16 || !D16x16) return LSSPA_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  DevBuf<double> buf;
  TRY(dev_alloc(ctx, buf, 64 + 64 + 256));
  hipError_t e = hipMemcpy(buf.ptr, A16x4, 64 * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(buf.ptr + 64, B4x16, 64 * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch_mfma_probe(buf.ptr, buf.ptr + 64, buf.ptr + 128, dtype == LSSPA_F32, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(D16x16, buf.ptr + 128, 256 * 8, hipMemcpyDeviceToHost);
  dev_free(buf);
  if (e != hipSuccess) return ctx->fail(LSSPA_ERR_HIP, "mfma probe", e);
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_factor(lsspa_ctx* ctx, const int32_t* perm, double* L, double* Lt, double* V, int32_t* p_pad,
                       int32_t* m_pad, int32_t* v_rows) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_STATE, "no problem loaded");
  HIPCHK(hipSetDevice(ctx->device));
  const size_t pp = ctx->p_pad, n_iblk = (ctx->p + NB - 1) / NB;
  if (p_pad) *p_pad = ctx->p_pad;
  if (m_pad) *m_pad = ctx->m_pad;
  if (v_rows) *v_rows = (int32_t)(n_iblk * NB);
  if (!perm) return LSSPA_OK;  // size query
  std::vector<char> seen;
  if (!is_permutation(perm, ctx->p, seen)) return ctx->fail(LSSPA_ERR_ARG, "perm is not a permutation");
  TRY(factor_identity(ctx, perm));
  const size_t ldv = (size_t)ldv_of(ctx->m_pad), mp = ctx->m_pad;
  // the device matrices are chunk-major; hand them out dense row-major
  auto unpack = [&](size_t mat_index, double* dst) -> int {
    std::vector<double> tmp(pp * pp);
    TRY(fetch_elems(ctx, ctx->lanes[0].A.ptr, mat_index * pp * pp, pp * pp, tmp.data()));
    for (size_t r = 0; r < pp; ++r)
      for (size_t c = 0; c < pp; ++c) dst[r * pp + c] = tmp[cm_off((int)pp, (int)r, (int)c)];
    return LSSPA_OK;
  };
  if (L) TRY(unpack(0, L));
  if (Lt && ctx->tri) TRY(unpack(1, Lt));
  if (V && vt_path(ctx)) {
    // the panel launches leave V^T (chunk-major, upper block triangle written; rows at or beyond p belong to no feature)
    const size_t rows = n_iblk * NB;
    std::vector<double> tmp(pp * pp);
    TRY(fetch_elems(ctx, ctx->lanes[0].V.ptr, 0, pp * pp, tmp.data()));
    for (size_t r = 0; r < rows; ++r)
      for (size_t c = 0; c < mp; ++c)
        V[r * mp + c] = (c / 128 > r / 128 || c >= (size_t)ctx->p) ? 0.0 : tmp[cm_off((int)pp, (int)c, (int)r)];
  } else if (V) {
    const size_t rows = n_iblk * NB;
    std::vector<double> tmp(rows * ldv);
    TRY(fetch_elems(ctx, ctx->lanes[0].V.ptr, 0, rows * ldv, tmp.data()));
    // tri: entries above a 128-column strip's first diagonal block are structurally zero and never written on the
    // device (strip2_kernel)
    for (size_t r = 0; r < rows; ++r)
      for (size_t c = 0; c < mp; ++c)
        V[r * mp + c] = (ctx->tri && r < (c / 128) * 128) ? 0.0 : tmp[r * ldv + c];
  }
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

}  // extern "C"

// ---- exact attribution by enumeration: the host path that k_subsets.hip and k_groups.hip share ---------------------
// n players (features, or groups of columns) and 2^n subsets, of which the kernels enumerate the n_high high ones in
// `units` workgroups of `per` each (EnumCut, which also holds how many steps one launch takes for either kind of
// player).  What differs between the entry points stays with them: their limits, which kernel runs and where a player's
// value goes in phi.  The selection calls and the K-fold CV calls go by the same pieces (best_run, top_run,
// rep_enumerate): a new call supplies its checks and its launcher, nothing else.
namespace {

// row length of the weight table [2][EXACT_MAX_PLAYERS + 1], which each kernel indexes with its own constant
constexpr int EXACT_MAX_PLAYERS = SUBSETS_MAX_P;
static_assert(SUBSETS_MAX_P == GROUPS_MAX_G, "the two enumerations share the layout of the Shapley weight table");
constexpr uint64_t EXACT_UNITS = 8192;
uint64_t exact_units(uint64_t n_high) { return std::min(n_high, EXACT_UNITS); }

// high subsets one enumeration launch of k_subsets.hip takes at most (over all units): ~35 ms of GPU time at p = 32
// 
constexpr uint64_t SUBSETS_PER_LAUNCH = 1ull << 20;
// One enumeration launch of k_groups.hip takes at most GROUPS_WORK_PER_LAUNCH units of work over all workgroups, a high
// subset counting as (rows of its matrix, on average)^2: the elimination of a subset costs that much per pivot row, and a
// subset of 64 columns several times one of 32.  2^26 is about 5 ms of one MI355X: far below the bound of
// 0.2 s, and long enough that the launches' own cost does not show.
constexpr uint64_t GROUPS_WORK_PER_LAUNCH = 1ull << 26;
// high subsets one launch takes at most over all its workgroups on the layout L
uint64_t groups_per_launch(const GroupLayout& L) {
  // rows of a subset's matrix: baseline and low columns always, the high columns half of the time
  const uint64_t rows = (uint64_t)(L.nb + L.ql + 1) + (uint64_t)(L.p - L.nb - L.ql + 1) / 2;
  return std::max<uint64_t>(1, GROUPS_WORK_PER_LAUNCH / (rows * rows));
}

static_assert(((1ull << (GROUPS_MAX_G - 1)) / EXACT_UNITS) <= (1ull << (GROUPS_BEST_CLASSES - 1)),
              "groups_best_kernel and groups_cv_best_kernel hold the size classes of the largest per: at most 31 high "
              "groups over EXACT_UNITS units");
// The cut of an enumeration: n_high high subsets in `units` workgroups of `per` each, `steps` of every unit a launch and
// so `launches` launches.  K: problems a step of a unit evaluates (the folds of the CV selection kernels), which divides
// the launch's bound; forced > 0: that many steps a launch instead (test hook).  steps is not cut to per: the launches
// are the same either way, and the one-problem plan hooks report it so; launch_steps() is what a launch takes.
struct EnumCut {
  uint64_t units, per, steps, launches;
  EnumCut(uint64_t n_high, uint64_t bound, int K, uint64_t forced) {
    units = exact_units(n_high);
    per = n_high / units;                                // both powers of two
    steps = forced ? forced : std::max<uint64_t>(1, bound / (units * (uint64_t)K));
    launches = (per + steps - 1) / steps;
  }
  explicit EnumCut(int p, int K = 1, uint64_t forced = 0)                   // the columns as players (k_subsets.hip)
      : EnumCut(1ull << (p - subsets_low_features(p)), SUBSETS_PER_LAUNCH, K, forced) {}
  explicit EnumCut(const GroupLayout& L, int K = 1, uint64_t forced = 0)    // the groups of a layout (k_groups.hip)
      : EnumCut(1ull << L.gh, groups_per_launch(L), K, forced) {}
  uint64_t launch_steps() const { return std::min(steps, per); }
};

// 1 / ||y||^2 of the replicate problems behind a, on the device: k_subsets.hip reads it there for every launch (one
// problem: one replicate), k_groups.hip for a launch of replicates (one problem: GroupArgs::inv_yy, the value)
inline void set_inv_yy(SubsetArgs& a, const double* on_device) { a.inv_yy = on_device; }
inline void set_inv_yy(GroupArgs& a, const double* on_device) { a.inv_yy_rep = on_device; }
// the relative pivot test of the exact paths (kernels.h, SubsetArgs::piv_tol)
inline double exact_piv_tol(int p) { return 16.0 * (double)p * 2.220446049250313e-16; }
// the layout's numbers as the kernels take them
inline void set_layout(GroupArgs& a, const GroupLayout& L) {
  a.p = L.p; a.ng = L.ng; a.nb = L.nb;
  a.gl = L.gl; a.gh = L.gh; a.ql = L.ql;
}
// caller masks (bit k = group k) -> the layout's numbering (low groups first)
std::vector<uint64_t> layout_masks(const GroupLayout& L, const uint64_t* masks, int64_t n) {
  std::vector<uint64_t> lay((size_t)n, 0);
  for (int64_t i = 0; i < n; ++i)
    for (int r = 0; r < L.ng; ++r)
      if ((masks[i] >> L.gid[r]) & 1ull) lay[i] |= 1ull << r;
  return lay;
}
// The kernels' view of replicate e0 of a dense store of problems (a bootstrap block, the folds, a block of the ridge
// path): G, H [.][p][p], g, h [.][p], inv_yy [.] and the info words [.] from there on, and the pivot test.  What else
// Args holds (the players, the weights, per, part) is the caller's.
template <typename Args>
void rep_view(Args& a, int p, int e0, const double* G, const double* g, const double* H, const double* h,
              const double* inv_yy, int32_t* info) {
  const size_t pp = (size_t)p * p;
  a.G = G + (size_t)e0 * pp;
  a.H = H + (size_t)e0 * pp;
  a.g = g + (size_t)e0 * p;
  a.h = h + (size_t)e0 * p;
  a.ldg = a.ldh = p;
  a.piv_tol = exact_piv_tol(p);
  set_inv_yy(a, inv_yy + e0);
  a.info = info + e0;
}

// The kernels' view of the loaded problem, the part that SubsetArgs and GroupArgs (Args) have in common: G, g, the test
// Gram (formed from the test factor in rect mode), the Shapley weights of n players by subset size, the tolerances and
// a cleared info word.  no_problem: the entry point's error for that; tab: GROUPS_TAB_LEN words to upload into W.tab
// beside the weights (nullptr: none).  The weight table carries three more rows, the interaction weights of n players
// (kernels.h, SubsetArgs::w), which only the interactions kernel reads.  1 / ||y||^2 lies behind the table on the device
// and is the caller's to set as its kernel takes it (subsets_args, groups_args).
constexpr int EXACT_W_ROWS = 5;
// w [EXACT_W_ROWS][EXACT_MAX_PLAYERS + 1]: the Shapley weights of n players by subset size (kernels.h, SubsetArgs::w)
void exact_weight_table(int n, double* w) {
  // w(k) = k! (n - 1 - k)! / n! = 1 / (n C(n - 1, k)); C(31, k) < 2^53 is exact in fp64
  constexpr int WR = EXACT_MAX_PLAYERS + 1;
  std::fill(w, w + EXACT_W_ROWS * WR, 0.0);
  double binom = 1.0;
  for (int k = 0; k < n; ++k) {
    const double wk = 1.0 / ((double)n * binom);
    w[WR + k] = wk;                      // wb[k]
    w[k + 1] = wk;                       // wa[k + 1]
    binom = binom * (double)(n - 1 - k) / (double)(k + 1);
  }
  // w2(s) = s! (n - 2 - s)! / (n - 1)! = 1 / ((n - 1) C(n - 2, s)), s = 0 .. n - 2; C(30, s) < 2^53 is exact in fp64.
  // By subset size k: gamma = w2(k), beta = w2(k - 1), alpha = w2(k - 2), each 0 outside 0 .. n - 2.
  double w2[EXACT_MAX_PLAYERS + 3] = {0.0};          // w2[s + 2]: alpha, beta read below 0 without a test
  binom = 1.0;
  for (int s = 0; s + 2 <= n; ++s) {
    w2[s + 2] = 1.0 / ((double)(n - 1) * binom);
    binom = binom * (double)(n - 2 - s) / (double)(s + 1);
  }
  for (int k = 0; k <= n; ++k) {
    const double al = w2[k], be = w2[k + 1], ga = w2[k + 2];
    w[2 * WR + k] = ga;
    w[3 * WR + k] = be + ga;
    w[4 * WR + k] = al + 2.0 * be + ga;
  }
}
template <typename Args>
int exact_view(lsspa_ctx* ctx, ExactWork& W, const char* no_problem, int n, const int32_t* tab, Args& a) {
  if (!ctx->have_problem) return ctx->fail(LSSPA_ERR_ARG, no_problem);
  const int p = ctx->p;
  HIPCHK(hipSetDevice(ctx->device));
  a = Args{};
  a.G = ctx->G.ptr;
  a.g = ctx->g.ptr;
  a.ldg = ctx->p_pad;
  if (ctx->tri) {
    a.H = ctx->H.ptr;
    a.h = ctx->h.ptr;
    a.ldh = ctx->p_pad;
  } else {
    TRY(dev_alloc(ctx, W.Hh, (size_t)p * p + p));
    HIPCHK(launch_subsets_test_gram(ctx->Ft.ptr, ctx->m_pad, ctx->ytil.ptr, p, ctx->m, W.Hh.ptr, ctx->stream));
    a.H = W.Hh.ptr;
    a.h = W.Hh.ptr + (size_t)p * p;
    a.ldh = p;
  }
  constexpr int WR = EXACT_MAX_PLAYERS + 1;
  double w[EXACT_W_ROWS * WR + 1];
  exact_weight_table(n, w);
  w[EXACT_W_ROWS * WR] = 1.0 / ctx->y_norm_sq;     // behind the table: what SubsetArgs::inv_yy points at
  TRY(dev_alloc(ctx, W.w, EXACT_W_ROWS * WR + 1));
  if (tab) TRY(dev_alloc(ctx, W.tab, GROUPS_TAB_LEN));
  TRY(dev_alloc(ctx, W.info, 8));
  HIPCHK(hipStreamSynchronize(ctx->stream));   // a previous call may still read W.w / W.tab; the copies are from host frames
  HIPCHK(hipMemcpy(W.w.ptr, w, sizeof w, hipMemcpyHostToDevice));
  if (tab) HIPCHK(hipMemcpy(W.tab.ptr, tab, GROUPS_TAB_LEN * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(W.info.ptr, 0, 8 * sizeof(int32_t), ctx->stream));
  a.w = W.w.ptr;
  a.piv_tol = exact_piv_tol(p);
  a.info = W.info.ptr;
  return LSSPA_OK;
}

struct Events {
  std::vector<hipEvent_t>& v;
  ~Events() {
    for (hipEvent_t e : v)
      if (e) (void)hipEventDestroy(e);
  }
};

// The launches of a cut on a stream, each between an event pair of its own: after the caller's synchronise read() gives
// the sum of the launches' own intervals, the longest of them and their number.  One timer serves all the launches of
// a call (the sets of replicates, the blocks of the ridge path).
struct LaunchTimer {
  std::vector<hipEvent_t> ev;
  Events guard{ev};
  // launch(s0, s1): steps s0 .. s1 - 1 of every unit
  template <typename Launch>
  int run(lsspa_ctx* ctx, const EnumCut& c, Launch&& launch) {
    size_t l = ev.size() / 2;
    ev.resize(ev.size() + 2 * (size_t)c.launches, nullptr);
    for (size_t k = 2 * l; k < ev.size(); ++k) HIPCHK(hipEventCreate(&ev[k]));
    for (uint64_t s0 = 0; s0 < c.per; s0 += c.steps, ++l) {
      HIPCHK(hipEventRecord(ev[2 * l], ctx->stream));
      HIPCHK(launch(s0, std::min(c.per, s0 + c.steps)));
      HIPCHK(hipEventRecord(ev[2 * l + 1], ctx->stream));
    }
    return LSSPA_OK;
  }
  int read(lsspa_ctx* ctx, double& total_ms, double& max_launch_ms, int64_t& launches) const {
    total_ms = max_launch_ms = 0.0;
    launches = (int64_t)(ev.size() / 2);
    for (size_t l = 0; l < ev.size() / 2; ++l) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, ev[2 * l], ev[2 * l + 1]));
      total_ms += ms;
      max_launch_ms = std::max(max_launch_ms, (double)ms);
    }
    return LSSPA_OK;
  }
};
// where a call's timing goes: lsspa_subsets_timing / lsspa_groups_timing, lsspa_cv_timing
int keep_timing(lsspa_ctx* ctx, ExactWork& W, const LaunchTimer& t) {
  return t.read(ctx, W.kernel_ms, W.max_launch_ms, W.launches);
}
int keep_timing(lsspa_ctx* ctx, CvWork& W, const LaunchTimer& t) {
  return t.read(ctx, W.enum_ms, W.max_launch_ms, W.launches);
}
// The end of every enumeration call on W (ExactWork, CvWork) once its result's copies are enqueued: the first n_info
// words of W.info into info (may be NULL), the synchronise, the launches' timing into W
template <typename Work>
int enum_finish(lsspa_ctx* ctx, Work& W, const LaunchTimer& t, int n_info, int32_t* info) {
  int32_t bits[CV_MAX_FOLDS] = {0};
  HIPCHK(hipMemcpyAsync(bits, W.info.ptr, sizeof(int32_t) * n_info, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (info) std::copy(bits, bits + n_info, info);
  return keep_timing(ctx, W, t);
}

// The enumeration that sums: launch(part, s0, s1) runs steps s0 .. s1 - 1 of every unit of the cut into the partial
// table part [units][cols].  out[0 .. cols - 1]: the table's column sums (launch_subsets_reduce).  With n players the
// first n + 1 columns are phi's: a player's phi is its column minus column n; what follows them is the entry point's
// own.  info (may be NULL): the info word.  Leaves the call's timing in W.
template <typename Launch>
int exact_enumerate(lsspa_ctx* ctx, ExactWork& W, int cols, const EnumCut& c, Launch&& launch, double* out,
                    int32_t* info) {
  TRY(dev_alloc(ctx, W.part, (size_t)c.units * cols));
  TRY(dev_alloc(ctx, W.out, (size_t)cols));
  HIPCHK(hipMemsetAsync(W.part.ptr, 0, sizeof(double) * c.units * cols, ctx->stream));
  LaunchTimer t;
  TRY(t.run(ctx, c, [&](uint64_t s0, uint64_t s1) { return launch(W.part.ptr, s0, s1); }));
  HIPCHK(launch_subsets_reduce(W.part.ptr, (int64_t)c.units, cols, W.out.ptr, ctx->stream));
  HIPCHK(hipMemcpyAsync(out, W.out.ptr, sizeof(double) * cols, hipMemcpyDeviceToHost, ctx->stream));
  return enum_finish(ctx, W, t, 1, info);
}

// ---- selection: the best model of every size, or the T best (lsspa_subsets_best / _top, lsspa_groups_best / _top and
// the four lsspa_cv_* selection calls) ----
// One skeleton each for the eight calls, on the buffers of W (ExactWork, CvWork) over n players (features, or groups:
// the masks are the caller's).  A call supplies its checks and its launcher, nothing else.
//
// best: every unit keeps its best model of every size 0 .. n, values in W.part [units][n + 1] and (mask, found) in
// W.best [units][n + 1][2], both cleared before the first launch; behind them in W.best the n + 1 pairs of the result,
// which launch_subsets_best_reduce takes over the units beside the values in W.out [n + 1].
// found[k] = the pair's flag, masks[k] = its mask (0 if none), v[k] = NaN if none: the n + 1 pairs mf of a result
void best_decode(const uint32_t* mf, int n, double* v, uint32_t* masks, uint8_t* found) {
  for (int k = 0; k <= n; ++k) {
    found[k] = mf[2 * k + 1] ? 1 : 0;
    masks[k] = found[k] ? mf[2 * k] : 0u;
    if (!found[k]) v[k] = std::nan("");
  }
}
// launch(s0, s1): steps s0 .. s1 - 1 of every unit into W.part and W.best; n_info: info words of the call
template <typename Work, typename Launch>
int best_run(lsspa_ctx* ctx, Work& W, const EnumCut& c, int n, int n_info, Launch&& launch, double* v, uint32_t* masks,
             uint8_t* found, int32_t* info) {
  hipStream_t st = ctx->stream;
  const size_t rows = (size_t)c.units * (n + 1);
  TRY(dev_alloc(ctx, W.part, rows));
  TRY(dev_alloc(ctx, W.out, (size_t)n + 1));
  TRY(dev_alloc(ctx, W.best, 2 * (rows + (size_t)n + 1)));
  HIPCHK(hipMemsetAsync(W.part.ptr, 0, sizeof(double) * rows, st));
  HIPCHK(hipMemsetAsync(W.best.ptr, 0, sizeof(uint32_t) * 2 * rows, st));
  LaunchTimer t;
  TRY(t.run(ctx, c, launch));
  uint32_t mf[2 * (EXACT_MAX_PLAYERS + 1)];
  uint32_t* out_m = W.best.ptr + 2 * rows;
  HIPCHK(launch_subsets_best_reduce(W.part.ptr, W.best.ptr, (int64_t)c.units, n, W.out.ptr, out_m, st));
  HIPCHK(hipMemcpyAsync(v, W.out.ptr, sizeof(double) * (n + 1), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(mf, out_m, sizeof(uint32_t) * 2 * (n + 1), hipMemcpyDeviceToHost, st));
  TRY(enum_finish(ctx, W, t, n_info, info));
  best_decode(mf, n, v, masks, found);
  return LSSPA_OK;
}

// top: every unit keeps per size a list of its T best, values in W.part [units][n + 1][T] (not cleared: no entry is read
// beyond a list's count) and in W.best the masks tm [units][n + 1][T], the counts tc [units][n + 1], cleared before the
// first launch, and behind them the result's masks out_m [n + 1][T] and counts out_c [n + 1], which
// launch_subsets_top_reduce merges from the units' lists beside the values in W.out [n + 1][T].
struct TopTable {
  int n, T;
  int sizes;                 // sizes one unit can hold: popc(s) + popc(t), s < per, t < 2^low, and no more than n + 1
  size_t rows;               // units (n + 1): lists in the table
  int64_t bytes;             // of the table: 12 a list entry (value, mask) and 4 a list (count)
  // low: the low players, which a unit enumerates at every step (q features, gl groups)
  TopTable(const EnumCut& c, int n_, int low, int T_)
      : n(n_), T(T_), sizes(std::min(n_, __builtin_popcountll(c.per - 1) + low) + 1), rows((size_t)c.units * (n_ + 1)),
        bytes((int64_t)rows * (12 * T_ + 4)) {}
  size_t n_out() const { return (size_t)(n + 1) * T; }
  size_t words() const { return rows * T + rows + n_out() + (size_t)n + 1; }      // of W.best
};
struct TopLists {
  uint32_t* tm;
  int32_t* tc;
  uint32_t* out_m;
  int32_t* out_c;
};
TopLists top_carve(const DevBuf<uint32_t>& best, const TopTable& t) {
  uint32_t* tm = best.ptr;
  uint32_t* out_m = tm + t.rows * t.T + t.rows;
  return {tm, reinterpret_cast<int32_t*>(tm + t.rows * t.T), out_m, reinterpret_cast<int32_t*>(out_m + t.n_out())};
}
// launch(tm, tc, s0, s1): steps s0 .. s1 - 1 of every unit into W.part and the lists; n_info: info words of the call
template <typename Work, typename Launch>
int top_run(lsspa_ctx* ctx, Work& W, const EnumCut& c, const TopTable& tab, int n_info, Launch&& launch, double* v,
            uint32_t* masks, int32_t* count, int32_t* info) {
  hipStream_t st = ctx->stream;
  const int n = tab.n, T = tab.T;
  TRY(dev_alloc(ctx, W.part, tab.rows * T));
  TRY(dev_alloc(ctx, W.out, tab.n_out()));
  TRY(dev_alloc(ctx, W.best, tab.words()));
  const TopLists b = top_carve(W.best, tab);
  HIPCHK(hipMemsetAsync(b.tc, 0, sizeof(int32_t) * tab.rows, st));
  LaunchTimer t;
  TRY(t.run(ctx, c, [&](uint64_t s0, uint64_t s1) { return launch(b.tm, b.tc, s0, s1); }));
  HIPCHK(launch_subsets_top_reduce(W.part.ptr, b.tm, b.tc, (int64_t)c.units, n, T, W.out.ptr, b.out_m, b.out_c, st));
  HIPCHK(hipMemcpyAsync(v, W.out.ptr, sizeof(double) * tab.n_out(), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(masks, b.out_m, sizeof(uint32_t) * tab.n_out(), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(count, b.out_c, sizeof(int32_t) * (n + 1), hipMemcpyDeviceToHost, st));
  return enum_finish(ctx, W, t, n_info, info);
}

// inter [n][n] of the column sums `out` of an interactions table of n players (kernels.h): I_ij = T0 - T1_i - T1_j +
// T2_ij off the diagonal, 0 on it, symmetric.  gid (may be NULL: the identity): the caller's number of player r, as
// GroupLayout::gid.  The one place where the index is formed: the one-problem calls and the bootstrap's share it.
void exact_inter_matrix(const double* out, int n, const int* gid, double* inter) {
  const double t0 = out[n + 1];
  const double* t1 = out + n + 2;
  const double* t2 = t1 + n;
  for (int i = 0; i < n; ++i) {
    const size_t gi = (size_t)(gid ? gid[i] : i);
    inter[gi * n + gi] = 0.0;
    for (int j = i + 1; j < n; ++j, ++t2) {
      const size_t gj = (size_t)(gid ? gid[j] : j);
      const double v = ((t0 - t1[i]) - t1[j]) + *t2;
      inter[gi * n + gj] = v;
      inter[gj * n + gi] = v;
    }
  }
}

// lsspa_subsets_timing, lsspa_groups_timing: kernel_ms is the sum of the launches' own event intervals (LaunchTimer), so
// the gaps between back-to-back launches do not count; max_launch_ms the longest of them, launches their number.
int exact_timing(const ExactWork& W, double* kernel_ms, double* max_launch_ms, int64_t* launches) {
  if (kernel_ms) *kernel_ms = W.kernel_ms;
  if (max_launch_ms) *max_launch_ms = W.max_launch_ms;
  if (launches) *launches = W.launches;
  return LSSPA_OK;
}

// test hook: vals[i] = the value of masks[i] (n > 0 of them, in the kernel's numbering) by launch(masks_d, vals_d);
// not_pd: the error when a subset's pivot failed
template <typename Launch>
int exact_debug_values(lsspa_ctx* ctx, ExactWork& W, const uint64_t* masks, int64_t n, double* vals, Launch&& launch,
                       const char* not_pd) {
  TRY(dev_alloc(ctx, W.masks, (size_t)n));
  TRY(dev_alloc(ctx, W.vals, (size_t)n));
  HIPCHK(hipMemcpy(W.masks.ptr, masks, sizeof(uint64_t) * n, hipMemcpyHostToDevice));
  HIPCHK(launch(W.masks.ptr, W.vals.ptr));
  HIPCHK(hipMemcpyAsync(vals, W.vals.ptr, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
  int32_t bits = 0;
  HIPCHK(hipMemcpyAsync(&bits, W.info.ptr, sizeof bits, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (bits & LSSPA_INFO_NOT_PD) return ctx->fail(LSSPA_ERR_STATE, not_pd);
  return LSSPA_OK;
}

// ---- ... by subset enumeration (k_subsets.hip) ----
int subsets_args(lsspa_ctx* ctx, SubsetArgs& a) {
  const int p = ctx->p;
  if (ctx->have_problem && p > SUBSETS_MAX_P) {   // (no problem loaded: exact_view says so)
    char msg[160];
    snprintf(msg, sizeof msg, "exact attribution by subsets takes at most p = %d features (this problem has %d)",
             SUBSETS_MAX_P, p);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  TRY(exact_view(ctx, ctx->sub, "no problem loaded (exact attribution by subsets)", p, nullptr, a));
  a.p = p;
  a.q = subsets_low_features(p);
  set_inv_yy(a, ctx->sub.w.ptr + EXACT_W_ROWS * (EXACT_MAX_PLAYERS + 1));
  return LSSPA_OK;
}

// lsspa_subsets_shapley and, with inter, lsspa_subsets_interactions: out receives the column sums of the partial
// table, p + 1 or subsets_inter_cols(p) of them (kernels.h).  Same units, launch splitting and timing for both.
int subsets_enumerate(lsspa_ctx* ctx, bool inter, double* out, int32_t* info) {
  SubsetArgs a;
  TRY(subsets_args(ctx, a));
  const int p = ctx->p;
  const EnumCut c(p);
  a.per = c.per;
  auto launch = [&](double* part, uint64_t s0, uint64_t s1) {
    a.part = part;
    return launch_subsets_enum(a, c.units, s0, s1, inter, ctx->stream);
  };
  return exact_enumerate(ctx, ctx->sub, inter ? subsets_inter_cols(p) : p + 1, c, launch, out, info);
}

// lsspa_subsets_best: the same cut and timing, best_run on ctx->sub
int subsets_best(lsspa_ctx* ctx, uint32_t include, double* v, uint32_t* masks, uint8_t* found, int32_t* info) {
  SubsetArgs a;
  TRY(subsets_args(ctx, a));
  const int p = ctx->p;
  if (p < 32 && (include >> p) != 0u) return ctx->fail(LSSPA_ERR_ARG, "include names a feature beyond p");
  const EnumCut c(p);
  a.per = c.per;
  ExactWork& W = ctx->sub;
  auto launch = [&](uint64_t s0, uint64_t s1) {
    a.part = W.part.ptr;
    return launch_subsets_best(a, c.units, s0, s1, include, W.best.ptr, ctx->stream);
  };
  return best_run(ctx, W, c, p, 1, launch, v, masks, found, info);
}

// lsspa_subsets_top: the same once more, top_run on ctx->sub
int subsets_top(lsspa_ctx* ctx, uint32_t include, int T, double* v, uint32_t* masks, int32_t* count, int32_t* info) {
  SubsetArgs a;
  TRY(subsets_args(ctx, a));
  const int p = ctx->p;
  if (p < 32 && (include >> p) != 0u) return ctx->fail(LSSPA_ERR_ARG, "include names a feature beyond p");
  if (T < 1 || T > SUBSETS_TOP_MAX) {
    char msg[120];
    snprintf(msg, sizeof msg, "lsspa_subsets_top keeps 1 .. %d subsets of every size (T = %d)", SUBSETS_TOP_MAX, T);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  const EnumCut c(p);
  a.per = c.per;
  ExactWork& W = ctx->sub;
  auto launch = [&](uint32_t* tm, int32_t* tc, uint64_t s0, uint64_t s1) {
    a.part = W.part.ptr;
    return launch_subsets_top(a, c.units, s0, s1, include, T, tm, tc, ctx->stream);
  };
  return top_run(ctx, W, c, TopTable(c, p, a.q, T), 1, launch, v, masks, count, info);
}

// ---- ... over groups of columns (k_groups.hip) ----
int groups_args(lsspa_ctx* ctx, const int32_t* labels, int32_t g, GroupArgs& a, GroupLayout& L) {
  const int p = ctx->p;
  char msg[200];
  L = GroupLayout{};
  if (ctx->have_problem) {   // (no problem loaded: exact_view says so)
    if (p > GROUPS_MAX_P) {
      snprintf(msg, sizeof msg, "exact attribution over groups takes at most p = %d columns (this problem has %d)",
               GROUPS_MAX_P, p);
      return ctx->fail(LSSPA_ERR_ARG, msg);
    }
    if (g > GROUPS_MAX_G) {
      snprintf(msg, sizeof msg, "exact attribution over groups takes at most g = %d groups (%d given)", GROUPS_MAX_G,
               (int)g);
      return ctx->fail(LSSPA_ERR_ARG, msg);
    }
    if (const char* why = groups_layout(labels, p, g, L)) {
      snprintf(msg, sizeof msg, "group labels: %s", why);
      return ctx->fail(LSSPA_ERR_ARG, msg);
    }
  }
  TRY(exact_view(ctx, ctx->grp, "no problem loaded (exact attribution over groups)", L.ng, L.tab, a));
  a.tab = ctx->grp.tab.ptr;
  set_layout(a, L);
  a.inv_yy = 1.0 / ctx->y_norm_sq;
  return LSSPA_OK;
}

// lsspa_groups_shapley and, with inter, lsspa_groups_interactions: the layout L of the labels, and in out the column
// sums of the partial table, g + 1 or subsets_inter_cols(g) of them in the layout's numbering (kernels.h).  Same units,
// launch splitting and timing for both.
int groups_enumerate(lsspa_ctx* ctx, bool inter, const int32_t* labels, int32_t g, GroupLayout& L, double* out,
                     int32_t* info) {
  GroupArgs a;
  TRY(groups_args(ctx, labels, g, a, L));
  const int ng = L.ng;
  const EnumCut c(L);
  a.per = c.per;
  auto launch = [&](double* part, uint64_t s0, uint64_t s1) {
    a.part = part;
    return launch_groups_enum(a, c.units, s0, s1, inter, ctx->stream);
  };
  return exact_enumerate(ctx, ctx->grp, inter ? subsets_inter_cols(ng) : ng + 1, c, launch, out, info);
}

// lsspa_groups_best: the same cut and timing, best_run on ctx->grp with the g groups as the players
int groups_best(lsspa_ctx* ctx, const int32_t* labels, int32_t g, double* u, uint32_t* masks, uint8_t* found,
                int32_t* info) {
  GroupArgs a;
  GroupLayout L;
  TRY(groups_args(ctx, labels, g, a, L));
  const EnumCut c(L);
  a.per = c.per;
  ExactWork& W = ctx->grp;
  auto launch = [&](uint64_t s0, uint64_t s1) {
    a.part = W.part.ptr;
    return launch_groups_best(a, L.gid, c.units, s0, s1, W.best.ptr, ctx->stream);
  };
  return best_run(ctx, W, c, L.ng, 1, launch, u, masks, found, info);
}

// lsspa_groups_top: the same once more, top_run on ctx->grp
int groups_top(lsspa_ctx* ctx, const int32_t* labels, int32_t g, int T, double* u, uint32_t* masks, int32_t* count,
               int32_t* info) {
  GroupArgs a;
  GroupLayout L;
  TRY(groups_args(ctx, labels, g, a, L));
  if (T < 1 || T > GROUPS_TOP_MAX) {
    char msg[120];
    snprintf(msg, sizeof msg, "lsspa_groups_top keeps 1 .. %d subsets of every size (T = %d)", GROUPS_TOP_MAX, T);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  const EnumCut c(L);
  a.per = c.per;
  ExactWork& W = ctx->grp;
  auto launch = [&](uint32_t* tm, int32_t* tc, uint64_t s0, uint64_t s1) {
    a.part = W.part.ptr;
    return launch_groups_top(a, L.gid, c.units, s0, s1, T, tm, tc, ctx->stream);
  };
  return top_run(ctx, W, c, TopTable(c, L.ng, L.gl, T), 1, launch, u, masks, count, info);
}

// ---- Owen value: the columns of a group, with the groups as coalition structure (k_groups.hip's header) ----
// The refined game of target group k (b columns) has g - 1 + b players: the other groups whole (the outer players) and
// the target's columns as singletons (the inner players), numbered in the caller's order with the target's columns in
// the target's place -- group l < k stays l, the target's columns become k .. k + b - 1 in column order, group l > k
// becomes l + b - 1.  groups_layout breaks ties between groups of one size by number, so the caller's numbering decides
// which players of a size are low.
constexpr int OWEN_MAX_PLAYERS = GROUPS_MAX_G;

// size [g] of the groups; false where groups_layout would refuse the labels (which then names the reason)
bool owen_sizes(const int32_t* labels, int p, int g, int* size) {
  if (!labels || g < 1 || g > GROUPS_MAX_G || p < 1 || p > GROUPS_MAX_P) return false;
  std::fill(size, size + g, 0);
  for (int j = 0; j < p; ++j) {
    if (labels[j] < -1 || labels[j] >= g) return false;
    if (labels[j] >= 0) ++size[labels[j]];
  }
  return std::all_of(size, size + g, [](int s) { return s > 0; });
}

// the first group whose refined game has more than OWEN_MAX_PLAYERS players (-1: none)
int owen_too_many(const int* size, int g) {
  for (int k = 0; k < g; ++k)
    if (g - 1 + size[k] > OWEN_MAX_PLAYERS) return k;
  return -1;
}

void owen_limit_message(char* msg, size_t n, int k, int b, int g) {
  snprintf(msg, n,
           "the Owen value enumerates the refined game of every group, the other g - 1 groups and the group's own "
           "columns, and takes at most %d players: group %d has %d columns beside %d other groups (%d players)",
           OWEN_MAX_PLAYERS, k, b, g - 1, g - 1 + b);
}

// The layout L of target k's refined game with the inner players marked in its table (GROUPS_TAB_OWEN_LO / _HI);
// ref [p]: the refined labels; n_lo, n_hi: the inner players among the low and the high groups.  (sizes as owen_sizes
// gives them and within the player limit: the refined labels are then good)
void owen_layout(const int32_t* labels, int p, int g, int k, int b, int32_t* ref, GroupLayout& L, int& n_lo, int& n_hi) {
  for (int j = 0, n = 0; j < p; ++j) {
    const int l = labels[j];
    ref[j] = l < k ? l : l > k ? l + b - 1 : k + n++;
  }
  (void)groups_layout(ref, p, g - 1 + b, L);
  uint32_t lo = 0, hi = 0;
  for (int r = 0; r < L.ng; ++r)
    if (L.gid[r] >= k && L.gid[r] < k + b) (r < L.gl ? lo : hi) |= 1u << (r < L.gl ? r : r - L.gl);
  L.tab[GROUPS_TAB_OWEN_LO] = (int32_t)lo;
  L.tab[GROUPS_TAB_OWEN_HI] = (int32_t)hi;      // gh <= 31: a layout of 32 high groups would have 7 x 32 columns
  n_lo = __builtin_popcount(lo);
  n_hi = __builtin_popcount(hi);
}

// rows 2 .. 4 of the weight table for launch_groups_owen: wo(r) of g groups, wi(t - 1) and wi(t) of b columns
void owen_weight_rows(int g, int b, double* w3) {
  constexpr int WR = EXACT_MAX_PLAYERS + 1;
  std::fill(w3, w3 + 3 * WR, 0.0);
  double binom = 1.0;                       // w(k) = 1 / (n C(n - 1, k)), as exact_weight_table forms it
  for (int r = 0; r < g; ++r) {
    w3[r] = 1.0 / ((double)g * binom);
    binom = binom * (double)(g - 1 - r) / (double)(r + 1);
  }
  binom = 1.0;
  for (int t = 0; t < b; ++t) {
    const double wt = 1.0 / ((double)b * binom);
    w3[WR + t + 1] = wt;                    // wi(t - 1) at t + 1
    w3[2 * WR + t] = wt;                    // wi(t)
    binom = binom * (double)(b - 1 - t) / (double)(t + 1);
  }
}

// One OWEN enumeration: the Owen values of target k's columns into owen[col]; bits: its info word
int owen_enumerate(lsspa_ctx* ctx, const int32_t* labels, int g, int k, int b, double* owen, int32_t* bits) {
  const int p = ctx->p;
  int32_t ref[GROUPS_MAX_P];
  GroupLayout L, marked;
  int n_lo, n_hi;
  owen_layout(labels, p, g, k, b, ref, marked, n_lo, n_hi);
  GroupArgs a;
  TRY(groups_args(ctx, ref, g - 1 + b, a, L));
  // what groups_args left on the device is the group game's of these labels: the marks and the Owen weights over it
  // (the stream is idle but for the clearing of the info word)
  constexpr int WR = EXACT_MAX_PLAYERS + 1;
  double w3[3 * WR];
  owen_weight_rows(g, b, w3);
  HIPCHK(hipMemcpy(ctx->grp.w.ptr + 2 * WR, w3, sizeof w3, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->grp.tab.ptr + GROUPS_TAB_OWEN_LO, marked.tab + GROUPS_TAB_OWEN_LO, 2 * sizeof(int32_t),
                   hipMemcpyHostToDevice));
  const int ng = L.ng;
  const EnumCut c(L);
  a.per = c.per;
  auto launch = [&](double* part, uint64_t s0, uint64_t s1) {
    a.part = part;
    return launch_groups_owen(a, c.units, s0, s1, ctx->stream);
  };
  double out[EXACT_MAX_PLAYERS + 1];
  TRY(exact_enumerate(ctx, ctx->grp, ng + 1, c, launch, out, bits));
  int col_of[OWEN_MAX_PLAYERS];             // refined label - k of an inner player -> its column
  for (int j = 0, n = 0; j < p; ++j)
    if (labels[j] == k) col_of[n++] = j;
  for (int r = 0; r < ng; ++r)
    if (L.gid[r] >= k && L.gid[r] < k + b) owen[col_of[L.gid[r] - k]] = out[r] - out[ng];
  return LSSPA_OK;
}

}  // namespace

extern "C" {

int lsspa_subsets_shapley(lsspa_ctx* ctx, double* phi, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!phi) return ctx->fail(LSSPA_ERR_ARG, "phi is NULL");
  double out[EXACT_MAX_PLAYERS + 1];
  TRY(subsets_enumerate(ctx, false, out, info));
  const int p = ctx->p;
  for (int j = 0; j < p; ++j) phi[j] = out[j] - out[p];
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_subsets_interactions(lsspa_ctx* ctx, double* phi, double* inter, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!phi || !inter) return ctx->fail(LSSPA_ERR_ARG, "phi / inter is NULL");
  std::vector<double> out((size_t)subsets_inter_cols(SUBSETS_MAX_P));
  TRY(subsets_enumerate(ctx, true, out.data(), info));
  const int p = ctx->p;
  for (int j = 0; j < p; ++j) phi[j] = out[j] - out[p];
  exact_inter_matrix(out.data(), p, nullptr, inter);
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_subsets_best(lsspa_ctx* ctx, uint32_t include, double* v, uint32_t* masks, uint8_t* found,
                       int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!v || !masks || !found) return ctx->fail(LSSPA_ERR_ARG, "v / masks / found is NULL");
  return subsets_best(ctx, include, v, masks, found, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_subsets_top(lsspa_ctx* ctx, uint32_t include, int32_t T, double* v, uint32_t* masks, int32_t* count,
                      int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!v || !masks || !count) return ctx->fail(LSSPA_ERR_ARG, "v / masks / count is NULL");
  return subsets_top(ctx, include, T, v, masks, count, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_subsets_top_plan(int32_t p, int32_t T, int64_t* plan) try {
  if (!plan || p < 1 || p > SUBSETS_MAX_P || T < 1 || T > SUBSETS_TOP_MAX) return LSSPA_ERR_ARG;
  const EnumCut c(p);
  const TopTable tab(c, p, subsets_low_features(p), T);
  const int64_t out[8] = {(int64_t)c.units, (int64_t)c.per, (int64_t)c.steps, (int64_t)c.launches, tab.sizes, tab.bytes,
                          T, 0};
  std::copy(out, out + 8, plan);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_NOMEM;
}

int lsspa_subsets_timing(const lsspa_ctx* ctx, double* kernel_ms, double* max_launch_ms, int64_t* launches) try {
  if (!ctx) return LSSPA_ERR_ARG;
  return exact_timing(ctx->sub, kernel_ms, max_launch_ms, launches);
} catch (...) {
  return abi_caught(const_cast<lsspa_ctx*>(ctx));
}

int lsspa_debug_subset_values(lsspa_ctx* ctx, const uint64_t* masks, int64_t n, double* v) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (n < 0 || (n > 0 && (!masks || !v))) return ctx->fail(LSSPA_ERR_ARG, "masks / v NULL or n < 0");
  SubsetArgs a;
  TRY(subsets_args(ctx, a));
  const uint64_t full = (1ull << ctx->p) - 1ull;     // p <= 32 here
  for (int64_t i = 0; i < n; ++i)
    if (masks[i] & ~full) return ctx->fail(LSSPA_ERR_ARG, "a mask names a feature beyond p");
  if (n == 0) return LSSPA_OK;
  auto launch = [&](const uint64_t* masks_d, double* vals_d) {
    return launch_subsets_debug(a, masks_d, n, vals_d, ctx->stream);
  };
  return exact_debug_values(ctx, ctx->sub, masks, n, v, launch, "a subset's Gram matrix is not positive definite");
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_groups_shapley(lsspa_ctx* ctx, const int32_t* labels, int32_t g, double* phi, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!phi || !labels) return ctx->fail(LSSPA_ERR_ARG, "labels / phi is NULL");
  GroupLayout L;
  double out[EXACT_MAX_PLAYERS + 1];
  TRY(groups_enumerate(ctx, false, labels, g, L, out, info));
  const int ng = L.ng;
  for (int r = 0; r < ng; ++r) phi[L.gid[r]] = out[r] - out[ng];
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_groups_interactions(lsspa_ctx* ctx, const int32_t* labels, int32_t g, double* phi, double* inter,
                              int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!phi || !inter || !labels) return ctx->fail(LSSPA_ERR_ARG, "labels / phi / inter is NULL");
  GroupLayout L;
  std::vector<double> out((size_t)subsets_inter_cols(GROUPS_MAX_G));
  TRY(groups_enumerate(ctx, true, labels, g, L, out.data(), info));
  const int ng = L.ng;
  for (int r = 0; r < ng; ++r) phi[L.gid[r]] = out[r] - out[ng];
  exact_inter_matrix(out.data(), ng, L.gid, inter);
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_groups_timing(const lsspa_ctx* ctx, double* kernel_ms, double* max_launch_ms, int64_t* launches) try {
  if (!ctx) return LSSPA_ERR_ARG;
  return exact_timing(ctx->grp, kernel_ms, max_launch_ms, launches);
} catch (...) {
  return abi_caught(const_cast<lsspa_ctx*>(ctx));
}

int lsspa_debug_group_values(lsspa_ctx* ctx, const int32_t* labels, int32_t g, const uint64_t* masks, int64_t n,
                             double* u) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!labels || n < 0 || (n > 0 && (!masks || !u))) return ctx->fail(LSSPA_ERR_ARG, "labels / masks / u NULL or n < 0");
  GroupArgs a;
  GroupLayout L;
  TRY(groups_args(ctx, labels, g, a, L));
  const uint64_t full = L.ng < 64 ? (1ull << L.ng) - 1ull : ~0ull;
  for (int64_t i = 0; i < n; ++i)
    if (masks[i] & ~full) return ctx->fail(LSSPA_ERR_ARG, "a mask names a group beyond g");
  if (n == 0) return LSSPA_OK;
  const std::vector<uint64_t> lay = layout_masks(L, masks, n);
  auto launch = [&](const uint64_t* masks_d, double* vals_d) {
    return launch_groups_debug(a, masks_d, n, vals_d, ctx->stream);
  };
  return exact_debug_values(ctx, ctx->grp, lay.data(), n, u, launch,
                            "a group subset's Gram matrix is not positive definite");
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_groups_best(lsspa_ctx* ctx, const int32_t* labels, int32_t g, double* u, uint32_t* masks, uint8_t* found,
                      int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!labels || !u || !masks || !found) return ctx->fail(LSSPA_ERR_ARG, "labels / u / masks / found is NULL");
  return groups_best(ctx, labels, g, u, masks, found, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_groups_best_plan(const int32_t* labels, int32_t p, int32_t g, int64_t* plan) try {
  GroupLayout L;
  if (!plan || g > GROUPS_MAX_G || p > GROUPS_MAX_P || groups_layout(labels, p, g, L)) return LSSPA_ERR_ARG;
  const EnumCut c(L);
  plan[0] = L.gl; plan[1] = L.gh; plan[2] = L.ql; plan[3] = L.nb;
  plan[4] = (int64_t)c.units;
  plan[5] = (int64_t)c.per;
  plan[6] = (int64_t)c.launches;
  plan[7] = __builtin_popcountll(c.per - 1) + 1;     // size classes of a unit: popc(s), s < per
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_ARG;
}

int lsspa_groups_top(lsspa_ctx* ctx, const int32_t* labels, int32_t g, int32_t T, double* u, uint32_t* masks,
                     int32_t* count, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!labels || !u || !masks || !count) return ctx->fail(LSSPA_ERR_ARG, "labels / u / masks / count is NULL");
  return groups_top(ctx, labels, g, T, u, masks, count, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_groups_top_plan(const int32_t* labels, int32_t p, int32_t g, int32_t T, int64_t* plan) try {
  GroupLayout L;
  if (!plan || g > GROUPS_MAX_G || p > GROUPS_MAX_P || T < 1 || T > GROUPS_TOP_MAX || groups_layout(labels, p, g, L))
    return LSSPA_ERR_ARG;
  const EnumCut c(L);
  const TopTable tab(c, L.ng, L.gl, T);
  const int64_t out[10] = {L.gl, L.gh, L.ql, L.nb, (int64_t)c.units, (int64_t)c.per, (int64_t)c.steps,
                           (int64_t)c.launches, tab.sizes, tab.bytes};
  std::copy(out, out + 10, plan);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_ARG;
}

int lsspa_groups_owen(lsspa_ctx* ctx, const int32_t* labels, int32_t g, double* owen, double* phi, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (!owen || !phi || !labels) return ctx->fail(LSSPA_ERR_ARG, "labels / owen / phi is NULL");
  // the player limit before any enumeration; labels that groups_layout refuses go on to lsspa_groups_shapley's refusal
  int size[GROUPS_MAX_G];
  const bool sized = ctx->have_problem && owen_sizes(labels, ctx->p, g, size);
  if (sized) {
    const int k = owen_too_many(size, g);
    if (k >= 0) {
      char msg[320];
      owen_limit_message(msg, sizeof msg, k, size[k], g);
      return ctx->fail(LSSPA_ERR_ARG, msg);
    }
  }
  GroupLayout L;
  double out[EXACT_MAX_PLAYERS + 1];
  int32_t bits = 0;
  TRY(groups_enumerate(ctx, false, labels, g, L, out, &bits));
  if (!sized) return ctx->fail(LSSPA_ERR_STATE, "lsspa_groups_owen: the labels passed the group game's checks only");
  for (int r = 0; r < L.ng; ++r) phi[L.gid[r]] = out[r] - out[L.ng];
  ExactWork& W = ctx->grp;
  double kernel_ms = W.kernel_ms, longest = W.max_launch_ms;
  int64_t launches = W.launches;
  const int p = ctx->p;
  for (int j = 0; j < p; ++j)
    if (labels[j] < 0) owen[j] = 0.0;
  for (int k = 0; k < g; ++k) {
    if (size[k] == 1) {
      for (int j = 0; j < p; ++j)
        if (labels[j] == k) owen[j] = phi[k];
      continue;
    }
    int32_t b1 = 0;
    TRY(owen_enumerate(ctx, labels, g, k, size[k], owen, &b1));
    bits |= b1;
    kernel_ms += W.kernel_ms;
    longest = std::max(longest, W.max_launch_ms);
    launches += W.launches;
  }
  W.kernel_ms = kernel_ms;
  W.max_launch_ms = longest;
  W.launches = launches;
  if (info) *info = bits;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_owen_plan(const int32_t* labels, int32_t p, int32_t g, int64_t* plan) try {
  int size[GROUPS_MAX_G];
  if (!plan || !owen_sizes(labels, p, g, size) || owen_too_many(size, g) >= 0) return LSSPA_ERR_ARG;
  for (int k = 0; k < g; ++k) {
    int32_t ref[GROUPS_MAX_P];
    GroupLayout L;
    int n_lo, n_hi;
    owen_layout(labels, p, g, k, size[k], ref, L, n_lo, n_hi);
    const EnumCut c(L);
    int64_t* row = plan + 8 * k;
    row[0] = L.ng; row[1] = L.gl; row[2] = L.gh; row[3] = L.ql;
    row[4] = n_lo; row[5] = n_hi;
    row[6] = (int64_t)(c.units * c.per);
    row[7] = size[k] == 1 ? 0 : (int64_t)c.launches;    // a group of one column: no enumeration of its own
  }
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_ARG;
}

}  // extern "C"

// ---- shared by the entry-point families below: rows onto the device, the reduced form of many responses -------------
namespace {

// The n rows of one side (X [n][ld], y [n]; dtype, location as lsspa_reduce's) to the caller's pack launch
// pack(src_x, src_y, rows, first_row) -> hipError_t, whose sources are on the device.  Rows on the device go in one
// launch.  Host rows go through the staging buffers, at most ~64 MB of X at a time, by plain copies on the context's
// stream; the stream is waited for after every chunk (the buffers are reused), not after rows from the device.  The
// staging buffers are the caller's to free.
template <typename Pack>
int load_rows(lsspa_ctx* ctx, DevBuf<char>& stage_x, DevBuf<char>& stage_y, const void* X, int64_t ld, const void* y,
              int64_t n, int32_t p, int32_t dtype, int32_t location, Pack&& pack) {
  if (location == LSSPA_DEVICE) {
    HIPCHK(pack(X, y, n, (int64_t)0));
    return LSSPA_OK;
  }
  const size_t esz = dtype == LSSPA_F32 ? 4 : 8;
  const int64_t rows = std::max<int64_t>(1, std::min<int64_t>(n, (64ll << 20) / (int64_t)(ld * esz)));
  TRY(dev_alloc(ctx, stage_x, (size_t)rows * ld * esz));
  TRY(dev_alloc(ctx, stage_y, (size_t)rows * esz));
  for (int64_t r0 = 0; r0 < n; r0 += rows) {
    const int64_t nr = std::min(rows, n - r0);
    const size_t xbytes = ((size_t)(nr - 1) * ld + p) * esz;     // the caller's last row ends with its column p - 1
    HIPCHK(hipMemcpyAsync(stage_x.ptr, (const char*)X + (size_t)r0 * ld * esz, xbytes, hipMemcpyHostToDevice,
                          ctx->stream));
    HIPCHK(hipMemcpyAsync(stage_y.ptr, (const char*)y + (size_t)r0 * esz, (size_t)nr * esz, hipMemcpyHostToDevice,
                          ctx->stream));
    HIPCHK(pack(stage_x.ptr, stage_y.ptr, nr, r0));
    HIPCHK(hipStreamSynchronize(ctx->stream));     // the staging buffers are reused
  }
  return LSSPA_OK;
}

// Every test response has a squared norm that is positive and finite; `text`: the caller's refusal, a format that may
// take the response's index
int reduced_check_yy(lsspa_ctx* ctx, int m, const double* yy, const char* text) {
  for (int r = 0; r < m; ++r)
    if (!(yy[r] > 0.0) || !std::isfinite(yy[r])) {
      char msg[160];
      snprintf(msg, sizeof msg, text, r);
      return ctx->fail(LSSPA_ERR_ARG, msg);
    }
  return LSSPA_OK;
}

// The reduced form (host arrays: G, H [p][p], g, h [m][p], yy [m], checked by reduced_check_yy) into F: the host
// copies, then G, H, g, h onto the device, allocated in that order.  g_dev, h_dev: where g and h go on the device (the
// permutation test keeps the observed pair beside F's, which are its replicates' slots).
int reduced_store(lsspa_ctx* ctx, ReducedForm& F, int p, int m, const double* G, const double* g, const double* H,
                  const double* h, const double* yy, DevBuf<double>& g_dev, DevBuf<double>& h_dev) {
  const size_t pp = (size_t)p * p, mp = (size_t)m * p;
  F.Gh.assign(G, G + pp);
  F.Hh.assign(H, H + pp);
  F.gh.assign(g, g + mp);
  F.hh.assign(h, h + mp);
  F.yyh.assign(yy, yy + m);
  TRY(dev_alloc(ctx, F.G, pp));
  TRY(dev_alloc(ctx, F.H, pp));
  TRY(dev_alloc(ctx, g_dev, mp));
  TRY(dev_alloc(ctx, h_dev, mp));
  HIPCHK(hipStreamSynchronize(ctx->stream));     // a previous call may still read the buffers
  HIPCHK(hipMemcpy(F.G.ptr, G, sizeof(double) * pp, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(F.H.ptr, H, sizeof(double) * pp, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(g_dev.ptr, g, sizeof(double) * mp, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h_dev.ptr, h, sizeof(double) * mp, hipMemcpyHostToDevice));
  F.p = p;
  F.m = m;
  return LSSPA_OK;
}

// the *_get_gram entry points: what was stored, each array only if asked for
void reduced_get(const ReducedForm& F, double* G, double* g, double* H, double* h, double* yy) {
  if (G) std::copy(F.Gh.begin(), F.Gh.end(), G);
  if (g) std::copy(F.gh.begin(), F.gh.end(), g);
  if (H) std::copy(F.Hh.begin(), F.Hh.end(), H);
  if (h) std::copy(F.hh.begin(), F.hh.end(), h);
  if (yy) std::copy(F.yyh.begin(), F.yyh.end(), yy);
}

}  // namespace

// ---- bootstrap of the exact attribution (k_boot.hip, boot_plan.cpp) ------------------------------------------------
// lsspa_boot_run cuts its R replicates into blocks (boot_plan: by memory).  A block: the weights of both sides on the
// device (counts drawn there, or the caller's rows copied), one weighted Gram pass per side, the fixed-order sum of its
// slices, finalise, and the enumeration of k_subsets.hip with the block's replicates as its second grid dimension.
// lsspa_boot_groups_run enumerates by k_groups.hip instead; the two interaction runs take the INTER instantiations of the
// same kernels and the interaction planners.  One block loop serves all four (boot_run_blocks).
namespace {

static_assert(EXACT_UNITS == BOOT_UNITS && SUBSETS_PER_LAUNCH == BOOT_SUBSETS_PER_LAUNCH && SUBSETS_MAX_P == BOOT_MAX_P,
              "boot_plan cuts the enumeration as exact_enumerate does");
static_assert(GROUPS_MAX_P == BOOT_GROUPS_MAX_P && GROUPS_MAX_G == BOOT_GROUPS_MAX_G && GROUPS_LOW_COLS == BOOT_LOW &&
                  GROUPS_WORK_PER_LAUNCH == BOOT_GROUPS_WORK_PER_LAUNCH,
              "boot_groups_plan cuts the enumeration as groups_enumerate does");

int boot_need_loaded(lsspa_ctx* ctx) {
  if (!ctx->boot.loaded) return ctx->fail(LSSPA_ERR_STATE, "no bootstrap data loaded (lsspa_boot_load comes first)");
  return LSSPA_OK;
}

// finite, >= 0, a positive sum in every replicate
int boot_check_weights(lsspa_ctx* ctx, const double* w, int64_t R, int64_t n, const char* name) {
  char msg[200];
  for (int64_t r = 0; r < R; ++r) {
    double sum = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      const double v = w[r * n + i];
      if (!(v >= 0.0) || !std::isfinite(v)) {
        snprintf(msg, sizeof msg, "%s[%lld][%lld] = %g: weights must be finite and >= 0", name, (long long)r,
                 (long long)i, v);
        return ctx->fail(LSSPA_ERR_ARG, msg);
      }
      sum += v;
    }
    if (!(sum > 0.0) || !std::isfinite(sum)) {
      snprintf(msg, sizeof msg, "%s: the weights of replicate %lld sum to %g (a positive finite sum is needed)", name,
               (long long)r, sum);
      return ctx->fail(LSSPA_ERR_ARG, msg);
    }
  }
  return LSSPA_OK;
}

// The plan of a run on the loaded rows without a layout of groups (the Gram side: lsspa_boot_debug_grams).  Up to p = 32
// that is boot_plan; beyond, the grouped planner with the columns as one group, whose Gram side is that of every layout.
const char* boot_rows_plan(const BootWork& B, int64_t R, int64_t block, BootPlan& P) {
  if (B.p <= BOOT_MAX_P) return boot_plan(R, B.n[0], B.n[1], B.p, block, P);
  return boot_groups_plan(R, B.n[0], B.n[1], B.p, 1, 1, 0, 0, block, P);
}

// ecols: the width of the enumeration's partial table (players + 1; the interaction runs: subsets_inter_cols(players))
int boot_alloc_block(lsspa_ctx* ctx, const BootPlan& P, const bool counts[2], bool enumerate, int ecols = 0) {
  BootWork& B = ctx->boot;
  const size_t blk = (size_t)P.block, c = (size_t)B.p + 1, p = (size_t)B.p;
  const size_t ec = ecols ? (size_t)ecols : c;
  for (int s = 0; s < 2; ++s) {
    if (counts[s])
      TRY(dev_alloc(ctx, B.cnt(s), blk * (size_t)B.n[s]));
    else
      TRY(dev_alloc(ctx, B.wt(s), blk * (size_t)B.n[s]));
    TRY(dev_alloc(ctx, B.part(s), (size_t)P.slices[s] * blk * P.pairs * 256));
    TRY(dev_alloc(ctx, B.S(s), blk * c * c));
  }
  TRY(dev_alloc(ctx, B.wsum, blk));
  if (!enumerate) return LSSPA_OK;
  TRY(dev_alloc(ctx, B.G, blk * p * p));
  TRY(dev_alloc(ctx, B.H, blk * p * p));
  TRY(dev_alloc(ctx, B.g, blk * p));
  TRY(dev_alloc(ctx, B.h, blk * p));
  TRY(dev_alloc(ctx, B.inv_yy, blk));
  TRY(dev_alloc(ctx, B.info, blk));
  TRY(dev_alloc(ctx, B.epart, (size_t)P.enum_reps * P.units * ec));
  TRY(dev_alloc(ctx, B.eout, blk * ec));
  TRY(dev_alloc(ctx, B.w, EXACT_W_ROWS * (EXACT_MAX_PLAYERS + 1)));
  return LSSPA_OK;
}

// The weights of replicates b0 .. b0 + nb - 1 of a run onto the device (w_host: the caller's [R][n] rows; NULL: counts
// of replicates r0 + b0 ..., or with `ones` weight 1 everywhere), then S [nb][c][c] of both sides and the sum of the
// training weights.  Nothing waits.  ev (may be NULL): events recorded after the counts and after the sums.
int boot_block_sums(lsspa_ctx* ctx, const BootPlan& P, const double* const w_host[2], bool ones, uint64_t seed,
                    uint64_t r0, int64_t b0, int nb, hipEvent_t after_counts) {
  BootWork& B = ctx->boot;
  hipStream_t st = ctx->stream;
  std::vector<double> one;
  for (int s = 0; s < 2; ++s) {
    if (w_host[s]) {
      HIPCHK(hipMemcpyAsync(B.wt(s).ptr, w_host[s] + b0 * B.n[s], sizeof(double) * (size_t)nb * B.n[s],
                            hipMemcpyHostToDevice, st));
    } else if (ones) {
      one.assign((size_t)nb * B.n[s], 1.0);
      HIPCHK(hipMemcpyAsync(B.wt(s).ptr, one.data(), sizeof(double) * one.size(), hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));        // `one` is reused for the other side
    } else {
      HIPCHK(launch_boot_counts(seed, r0 + (uint64_t)b0, s, B.n[s], nb, B.cnt(s).ptr, st));
    }
  }
  if (after_counts) HIPCHK(hipEventRecord(after_counts, st));
  for (int s = 0; s < 2; ++s) {
    const bool counts = !w_host[s] && !ones;
    const uint32_t* cnt = counts ? B.cnt(s).ptr : nullptr;
    const double* wt = counts ? nullptr : B.wt(s).ptr;
    HIPCHK(launch_boot_gram(P, s, B.Z(s).ptr, B.n[s], cnt, wt, nb, B.part(s).ptr, st));
    if (s == 0) HIPCHK(launch_boot_wsum(cnt, wt, B.n[s], nb, B.wsum.ptr, st));
    HIPCHK(launch_boot_reduce(P, s, B.part(s).ptr, B.p, nb, B.S(s).ptr, st));
  }
  return LSSPA_OK;
}

// R^2 of the full model of one replicate on the host: theta = G^-1 g by Cholesky, (2 theta.h - theta.H theta) / ||y||^2;
// NaN where G is not positive definite
double boot_r2(int p, const double* G, const double* g, const double* H, const double* h, double inv_yy) {
  double L[SUBSETS_MAX_P * SUBSETS_MAX_P], t[SUBSETS_MAX_P];
  for (int j = 0; j < p; ++j) {
    double d = G[j * p + j];
    for (int k = 0; k < j; ++k) d -= L[j * p + k] * L[j * p + k];
    if (!(d > 0.0)) return std::nan("");
    const double l = std::sqrt(d);
    L[j * p + j] = l;
    for (int i = j + 1; i < p; ++i) {
      double v = G[i * p + j];
      for (int k = 0; k < j; ++k) v -= L[i * p + k] * L[j * p + k];
      L[i * p + j] = v / l;
    }
  }
  for (int i = 0; i < p; ++i) {
    double v = g[i];
    for (int k = 0; k < i; ++k) v -= L[i * p + k] * t[k];
    t[i] = v / L[i * p + i];
  }
  for (int i = p - 1; i >= 0; --i) {
    double v = t[i];
    for (int k = i + 1; k < p; ++k) v -= L[k * p + i] * t[k];
    t[i] = v / L[i * p + i];
  }
  double lin = 0.0, quad = 0.0;
  for (int i = 0; i < p; ++i) {
    lin += t[i] * h[i];
    double v = 0.0;
    for (int j = 0; j < p; ++j) v += H[i * p + j] * t[j];
    quad += t[i] * v;
  }
  return (2.0 * lin - quad) * inv_yy;
}

// The same over the columns cols[0 .. k-1] of a problem of p columns (p <= GROUPS_MAX_P): R^2 of the model on those
// columns alone; 0 for k = 0.  ws: the caller's workspace, grown here.  boot_r2 is kept beside it as it was: its
// arrays stop at SUBSETS_MAX_P, and lsspa_boot_run's r2 keeps the bits it had (the compiler contracts the two
// index forms into fused operations as it sees fit).
double boot_r2_cols(int p, const int* cols, int k, const double* G, const double* g, const double* H, const double* h,
                    double inv_yy, std::vector<double>& ws) {
  if (k == 0) return 0.0;
  if (ws.size() < (size_t)k * k + k) ws.resize((size_t)k * k + k);
  double *L = ws.data(), *t = ws.data() + (size_t)k * k;
  for (int j = 0; j < k; ++j) {
    double d = G[cols[j] * p + cols[j]];
    for (int q = 0; q < j; ++q) d -= L[j * k + q] * L[j * k + q];
    if (!(d > 0.0)) return std::nan("");
    const double l = std::sqrt(d);
    L[j * k + j] = l;
    for (int i = j + 1; i < k; ++i) {
      double v = G[cols[i] * p + cols[j]];
      for (int q = 0; q < j; ++q) v -= L[i * k + q] * L[j * k + q];
      L[i * k + j] = v / l;
    }
  }
  for (int i = 0; i < k; ++i) {
    double v = g[cols[i]];
    for (int q = 0; q < i; ++q) v -= L[i * k + q] * t[q];
    t[i] = v / L[i * k + i];
  }
  for (int i = k - 1; i >= 0; --i) {
    double v = t[i];
    for (int q = i + 1; q < k; ++q) v -= L[q * k + i] * t[q];
    t[i] = v / L[i * k + i];
  }
  double lin = 0.0, quad = 0.0;
  for (int i = 0; i < k; ++i) {
    lin += t[i] * h[cols[i]];
    double v = 0.0;
    for (int j = 0; j < k; ++j) v += H[cols[i] * p + cols[j]] * t[j];
    quad += t[i] * v;
  }
  return (2.0 * lin - quad) * inv_yy;
}

// lsspa_boot_load and lsspa_boot_groups_load: the rows of both sides into Z [n][ldz]; P: a plan for these rows
int boot_load_rows(lsspa_ctx* ctx, const BootPlan& P, const char* name, const void* X_train, int64_t ld_train,
                   const void* y_train, int64_t N, const void* X_test, int64_t ld_test, const void* y_test, int64_t M,
                   int32_t p, double reg, int32_t dtype, int32_t location) {
  if (!X_train || !y_train || !X_test || !y_test || ld_train < p || ld_test < p || !std::isfinite(reg) ||
      (dtype != LSSPA_F64 && dtype != LSSPA_F32) || (location != LSSPA_HOST && location != LSSPA_DEVICE)) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: NULL array, ld < p, reg not finite, or bad dtype / location", name);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  HIPCHK(hipSetDevice(ctx->device));
  BootWork& B = ctx->boot;
  B.loaded = false;
  const void* X[2] = {X_train, X_test};
  const void* y[2] = {y_train, y_test};
  const int64_t n[2] = {N, M}, ld[2] = {ld_train, ld_test};
  for (int s = 0; s < 2; ++s) {
    TRY(dev_alloc(ctx, B.Z(s), (size_t)n[s] * P.ldz));
    TRY(load_rows(ctx, B.stage_x, B.stage_y, X[s], ld[s], y[s], n[s], p, dtype, location,
                  [&](const void* sx, const void* sy, int64_t nr, int64_t r0) {
                    return launch_boot_pack(sx, ld[s], sy, nr, p, dtype == LSSPA_F32, B.Z(s).ptr, P.ldz, r0,
                                            ctx->stream);
                  }));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  dev_free(B.stage_x);
  dev_free(B.stage_y);
  B.p = p;
  B.n[0] = N;
  B.n[1] = M;
  B.reg = reg;
  B.loaded = true;
  return LSSPA_OK;
}

// the fifteen numbers of the debug entry points (include/lsspa.h, lsspa_debug_boot_plan)
void boot_plan15(const BootPlan& P, int64_t* plan15) {
  const int64_t v[15] = {P.cb, P.ldz, P.pairs, P.rpw, P.rps[0], P.rps[1], P.slices[0], P.slices[1], P.rep_bytes,
                         P.block, P.n_blocks, P.enum_reps, (int64_t)P.units, (int64_t)P.per, (int64_t)P.steps};
  std::copy(v, v + 15, plan15);
}

// The Shapley weights of `players` players -- and with tab the layout of the groups -- onto the device, for a run
int boot_upload_tables(lsspa_ctx* ctx, int players, const int32_t* tab) {
  BootWork& B = ctx->boot;
  if (tab) TRY(dev_alloc(ctx, B.tab, GROUPS_TAB_LEN));
  double w[EXACT_W_ROWS * (EXACT_MAX_PLAYERS + 1)];
  exact_weight_table(players, w);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpy(B.w.ptr, w, sizeof w, hipMemcpyHostToDevice));
  if (tab) HIPCHK(hipMemcpy(B.tab.ptr, tab, GROUPS_TAB_LEN * sizeof(int32_t), hipMemcpyHostToDevice));
  return LSSPA_OK;
}

// The block loop of the four run functions (phi or interactions, features or groups).  Per block of P.block replicates:
// weights, the weighted Grams and their sums, finalise, then the enumeration in launches of P.enum_reps replicates and
// P.steps steps into a partial table `cols` wide, its reduction to a row of `ocols` doubles a replicate, and the block's
// results on the host.  What differs stays with the entry point:
//   launch(e0, ne, s0, s1): steps s0 .. s1 - 1 of replicates e0 .. e0 + ne - 1 of the block into B.epart;
//   reduce(e0, ne): the table of those replicates into rows e0 .. e0 + ne - 1 of B.eout [block][ocols] (the sums: the
//     table's column sums, boot_column_sums below; the best run: the best over the units);
//   emit(r, out, G, g, H, h, inv_yy): replicate r of the run from its row of B.eout and its reduced problem (host).
// The buffers are the caller's (boot_alloc_block with this P and cols, boot_upload_tables).  Leaves the run's timing in
// B.ms.
template <typename Launch, typename Reduce, typename Emit>
int boot_run_blocks(lsspa_ctx* ctx, const BootPlan& P, int64_t R, uint64_t seed, int64_t first,
                    const double* const w_host[2], int cols, int ocols, Launch&& launch, Reduce&& reduce, Emit&& emit,
                    int32_t* info) {
  BootWork& B = ctx->boot;
  hipStream_t st = ctx->stream;
  const int p = B.p;
  const size_t c = (size_t)cols, oc = (size_t)ocols;
  std::vector<hipEvent_t> ev(4, nullptr);
  Events guard{ev};
  for (hipEvent_t& e : ev) HIPCHK(hipEventCreate(&e));
  std::vector<double> out((size_t)P.block * oc), Gh((size_t)P.block * p * p), Hh((size_t)P.block * p * p),
      gh((size_t)P.block * p), hh((size_t)P.block * p), yh((size_t)P.block);
  B.ms[0] = B.ms[1] = B.ms[2] = 0.0;
  for (int64_t b0 = 0; b0 < R; b0 += P.block) {
    const int nb = (int)std::min<int64_t>(P.block, R - b0);
    HIPCHK(hipEventRecord(ev[0], st));
    TRY(boot_block_sums(ctx, P, w_host, false, seed, (uint64_t)first, b0, nb, ev[1]));
    HIPCHK(launch_boot_finalize(B.S0.ptr, B.S1.ptr, B.wsum.ptr, p, B.reg, nb, B.G.ptr, B.g.ptr, B.H.ptr, B.h.ptr,
                                B.inv_yy.ptr, st));
    HIPCHK(hipEventRecord(ev[2], st));
    HIPCHK(hipMemsetAsync(B.info.ptr, 0, sizeof(int32_t) * nb, st));
    for (int e0 = 0; e0 < nb; e0 += (int)P.enum_reps) {
      const int ne = std::min<int>((int)P.enum_reps, nb - e0);
      HIPCHK(hipMemsetAsync(B.epart.ptr, 0, sizeof(double) * (size_t)ne * P.units * c, st));
      for (uint64_t s0 = 0; s0 < P.per; s0 += P.steps) HIPCHK(launch(e0, ne, s0, std::min(P.per, s0 + P.steps)));
      HIPCHK(reduce(e0, ne));
    }
    HIPCHK(hipEventRecord(ev[3], st));
    HIPCHK(hipMemcpyAsync(out.data(), B.eout.ptr, sizeof(double) * (size_t)nb * oc, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(info + b0, B.info.ptr, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(Gh.data(), B.G.ptr, sizeof(double) * (size_t)nb * p * p, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(Hh.data(), B.H.ptr, sizeof(double) * (size_t)nb * p * p, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(gh.data(), B.g.ptr, sizeof(double) * (size_t)nb * p, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hh.data(), B.h.ptr, sizeof(double) * (size_t)nb * p, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(yh.data(), B.inv_yy.ptr, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int r = 0; r < nb; ++r)
      emit(b0 + r, &out[(size_t)r * oc], &Gh[(size_t)r * p * p], &gh[(size_t)r * p], &Hh[(size_t)r * p * p],
           &hh[(size_t)r * p], yh[r]);
    for (int k = 0; k < 3; ++k) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
      B.ms[k] += ms;
    }
  }
  return LSSPA_OK;
}

// the reduce step of the runs that sum: the column sums of the table of replicates e0 .. e0 + ne - 1, `cols` wide
auto boot_column_sums(lsspa_ctx* ctx, const BootPlan& P, int cols) {
  return [ctx, &P, cols](int e0, int ne) {
    BootWork& B = ctx->boot;
    return launch_subsets_reduce(B.epart.ptr, (int64_t)P.units, cols, B.eout.ptr + (size_t)e0 * cols, ctx->stream, ne);
  };
}

// The weights of a run: the caller's [R][n] rows of a side, or NULL and counts drawn on the device
struct BootWeights {
  const double* w_host[2];
  bool counts[2];
};

// What every run does between its plan and its first allocation: the planner's refusal `why` (NULL: none) under the
// entry point's name, the caller's weights, the device
int boot_begin(lsspa_ctx* ctx, const char* name, const char* why, int64_t R, const double* w_train, const double* w_test,
               BootWeights& W) {
  BootWork& B = ctx->boot;
  if (why) {
    char msg[240];
    snprintf(msg, sizeof msg, "%s: %s", name, why);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  if (w_train) TRY(boot_check_weights(ctx, w_train, R, B.n[0], "w_train"));
  if (w_test) TRY(boot_check_weights(ctx, w_test, R, B.n[1], "w_test"));
  HIPCHK(hipSetDevice(ctx->device));
  W = BootWeights{{w_train, w_test}, {!w_train, !w_test}};
  return LSSPA_OK;
}

// labels / g of a grouped run against the loaded columns; too_many: the entry point's refusal of g > GROUPS_MAX_G
int boot_layout(lsspa_ctx* ctx, const int32_t* labels, int32_t g, const char* too_many, GroupLayout& L) {
  char msg[240];
  if (g > GROUPS_MAX_G) {
    snprintf(msg, sizeof msg, too_many, GROUPS_MAX_G, (int)g);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  if (const char* why = groups_layout(labels, ctx->boot.p, g, L)) {
    snprintf(msg, sizeof msg, "group labels: %s", why);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  return LSSPA_OK;
}

// k_subsets.hip's view of the block's replicates from e0 on (one launch's: the kernels' second grid dimension)
SubsetArgs boot_subset_args(const BootWork& B, const BootPlan& P, int e0) {
  SubsetArgs a{};
  a.p = B.p;
  a.q = subsets_low_features(B.p);
  a.w = B.w.ptr;
  a.per = P.per;
  a.part = B.epart.ptr;
  rep_view(a, B.p, e0, B.G.ptr, B.g.ptr, B.H.ptr, B.h.ptr, B.inv_yy.ptr, B.info.ptr);
  return a;
}

// the same of k_groups.hip, over the layout L
GroupArgs boot_group_args(const BootWork& B, const BootPlan& P, const GroupLayout& L, int e0) {
  GroupArgs a{};
  set_layout(a, L);
  a.w = B.w.ptr;
  a.tab = B.tab.ptr;
  a.per = P.per;
  a.part = B.epart.ptr;
  rep_view(a, B.p, e0, B.G.ptr, B.g.ptr, B.H.ptr, B.h.ptr, B.inv_yy.ptr, B.info.ptr);
  return a;
}

// r2 and r2_base of a replicate of a grouped run, by boot_r2_cols: the model on all p columns, and on the baseline's,
// the layout's first nb
struct BootGroupR2 {
  int p, nb;
  int all[GROUPS_MAX_P], base[GROUPS_MAX_P];
  std::vector<double> ws;
  BootGroupR2(int p_, const GroupLayout& L) : p(p_), nb(L.nb) {
    for (int j = 0; j < p; ++j) all[j] = j;
    for (int j = 0; j < nb; ++j) base[j] = L.tab[GROUPS_TAB_COLS + j];
  }
  void operator()(const double* G, const double* g, const double* H, const double* h, double inv_yy, double& r2,
                  double& r2_base) {
    r2 = boot_r2_cols(p, all, p, G, g, H, h, inv_yy, ws);
    r2_base = boot_r2_cols(p, base, nb, G, g, H, h, inv_yy, ws);
  }
};

// lsspa_boot_run and, with inter, lsspa_boot_interactions_run: the enumeration of k_subsets.hip over the block's
// replicates; `name` is the entry point's
int boot_subsets_run(lsspa_ctx* ctx, const char* name, int64_t R, uint64_t seed, int64_t first, const double* w_train,
                     const double* w_test, int64_t block, double* phi, double* inter, double* r2, int32_t* info) {
  BootWork& B = ctx->boot;
  const int p = B.p;
  if (p > SUBSETS_MAX_P) {
    char msg[240];
    snprintf(msg, sizeof msg, "%s enumerates feature subsets and takes at most p = %d features (%d loaded by "
             "lsspa_boot_groups_load: %s attributes to groups of them)", name, SUBSETS_MAX_P, p,
             inter ? "lsspa_boot_groups_interactions_run" : "lsspa_boot_groups_run");
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  BootPlan P;
  BootWeights W;
  TRY(boot_begin(ctx, name, inter ? boot_inter_plan(R, B.n[0], B.n[1], p, block, P)
                                  : boot_plan(R, B.n[0], B.n[1], p, block, P), R, w_train, w_test, W));
  const int cols = inter ? subsets_inter_cols(p) : p + 1;
  TRY(boot_alloc_block(ctx, P, W.counts, true, cols));
  TRY(boot_upload_tables(ctx, p, nullptr));
  auto launch = [&](int e0, int ne, uint64_t s0, uint64_t s1) {
    return launch_subsets_enum(boot_subset_args(B, P, e0), P.units, s0, s1, inter != nullptr, ctx->stream, ne);
  };
  auto emit = [&](int64_t r, const double* out, const double* G, const double* g, const double* H, const double* h,
                  double inv_yy) {
    for (int j = 0; j < p; ++j) phi[r * p + j] = out[j] - out[p];
    if (inter) exact_inter_matrix(out, p, nullptr, inter + (size_t)r * p * p);
    r2[r] = boot_r2(p, G, g, H, h, inv_yy);
  };
  return boot_run_blocks(ctx, P, R, seed, first, W.w_host, cols, cols, launch, boot_column_sums(ctx, P, cols), emit,
                         info);
}

// lsspa_boot_groups_run and, with inter, lsspa_boot_groups_interactions_run: the enumeration of k_groups.hip
int boot_groups_run(lsspa_ctx* ctx, const char* name, const int32_t* labels, int32_t g, int64_t R, uint64_t seed,
                    int64_t first, const double* w_train, const double* w_test, int64_t block, double* phi,
                    double* inter, double* r2, double* r2_base, int32_t* info) {
  BootWork& B = ctx->boot;
  GroupLayout L;
  TRY(boot_layout(ctx, labels, g, "the bootstrap over groups of columns takes at most g = %d groups (%d given)", L));
  BootPlan P;
  BootWeights W;
  TRY(boot_begin(ctx, name, inter ? boot_groups_inter_plan(R, B.n[0], B.n[1], B.p, L.ng, L.gh, L.nb, L.ql, block, P)
                                  : boot_groups_plan(R, B.n[0], B.n[1], B.p, L.ng, L.gh, L.nb, L.ql, block, P),
                 R, w_train, w_test, W));
  const int ng = L.ng, cols = inter ? subsets_inter_cols(ng) : ng + 1;
  TRY(boot_alloc_block(ctx, P, W.counts, true, cols));
  TRY(boot_upload_tables(ctx, ng, L.tab));
  BootGroupR2 fit(B.p, L);
  auto launch = [&](int e0, int ne, uint64_t s0, uint64_t s1) {
    return launch_groups_enum(boot_group_args(B, P, L, e0), P.units, s0, s1, inter != nullptr, ctx->stream, ne);
  };
  auto emit = [&](int64_t r, const double* out, const double* G, const double* gv, const double* H, const double* h,
                  double inv_yy) {
    for (int k = 0; k < ng; ++k) phi[r * ng + L.gid[k]] = out[k] - out[ng];
    if (inter) exact_inter_matrix(out, ng, L.gid, inter + (size_t)r * ng * ng);
    fit(G, gv, H, h, inv_yy, r2[r], r2_base[r]);
  };
  return boot_run_blocks(ctx, P, R, seed, first, W.w_host, cols, cols, launch, boot_column_sums(ctx, P, cols), emit,
                         info);
}

// What the two best-subset runs do after their plan, over n players (features, or groups with their table `tab`).  The
// table is best_run's, once per replicate of a launch: values in B.epart [enum_reps][units][n + 1], (mask, found) in
// B.ebest [enum_reps][units][n + 1][2], cleared before a set of replicates' first launch; a replicate's row of B.eout is
// 2 (n + 1) doubles wide, the best values and behind them the n + 1 (mask, found) pairs as launch_subsets_best_reduce
// writes them (8 bytes a pair), which best_decode reads.
//   launch(e0, ne, s0, s1): as boot_run_blocks', the kernel that also writes B.ebest;
//   fit(r, G, g, H, h, inv_yy): the run's r2 entries of replicate r.
template <typename Launch, typename Fit>
int boot_best_blocks(lsspa_ctx* ctx, const BootPlan& P, const BootWeights& W, int64_t R, uint64_t seed, int64_t first,
                     int n, const int32_t* tab, Launch&& launch, Fit&& fit, double* v, uint32_t* masks, uint8_t* found,
                     int32_t* info) {
  BootWork& B = ctx->boot;
  const int n1 = n + 1;
  TRY(boot_alloc_block(ctx, P, W.counts, true, n1));
  TRY(dev_alloc(ctx, B.eout, (size_t)P.block * 2 * n1));
  const size_t rows = (size_t)P.units * n1;                // entries of one replicate's table
  TRY(dev_alloc(ctx, B.ebest, 2 * rows * (size_t)P.enum_reps));
  TRY(boot_upload_tables(ctx, n, tab));
  auto cleared = [&](int e0, int ne, uint64_t s0, uint64_t s1) {
    if (s0 == 0) {      // a new set of replicates: nothing found yet
      hipError_t e = hipMemsetAsync(B.ebest.ptr, 0, sizeof(uint32_t) * 2 * rows * (size_t)ne, ctx->stream);
      if (e != hipSuccess) return e;
    }
    return launch(e0, ne, s0, s1);
  };
  auto reduce = [&](int e0, int ne) {
    double* row = B.eout.ptr + (size_t)e0 * 2 * n1;
    return launch_subsets_best_reduce(B.epart.ptr, B.ebest.ptr, (int64_t)P.units, n, row,
                                      reinterpret_cast<uint32_t*>(row + n1), ctx->stream, ne, 2 * n1);
  };
  auto emit = [&](int64_t r, const double* out, const double* G, const double* g, const double* H, const double* h,
                  double inv_yy) {
    uint32_t mf[2 * (EXACT_MAX_PLAYERS + 1)];
    std::memcpy(mf, out + n1, sizeof(uint32_t) * 2 * n1);
    std::copy(out, out + n1, v + r * n1);
    best_decode(mf, n, v + r * n1, masks + r * n1, found + r * n1);
    fit(r, G, g, H, h, inv_yy);
  };
  return boot_run_blocks(ctx, P, R, seed, first, W.w_host, n1, 2 * n1, cleared, reduce, emit, info);
}

// lsspa_boot_best_run: subsets_best_kernel's replicates over the block's reduced problems
int boot_best_run(lsspa_ctx* ctx, int64_t R, uint64_t seed, int64_t first, const double* w_train, const double* w_test,
                  int64_t block, uint32_t include, double* v, uint32_t* masks, uint8_t* found, double* r2,
                  int32_t* info) {
  BootWork& B = ctx->boot;
  const int p = B.p;
  if (p > SUBSETS_MAX_P) {
    char msg[240];
    snprintf(msg, sizeof msg, "lsspa_boot_best_run enumerates feature subsets and takes at most p = %d features (%d "
             "loaded by lsspa_boot_groups_load)", SUBSETS_MAX_P, p);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  if (p < 32 && (include >> p) != 0u) return ctx->fail(LSSPA_ERR_ARG, "include names a feature beyond p");
  BootPlan P;
  BootWeights W;
  TRY(boot_begin(ctx, "lsspa_boot_best_run", boot_best_plan(R, B.n[0], B.n[1], p, block, P), R, w_train, w_test, W));
  auto launch = [&](int e0, int ne, uint64_t s0, uint64_t s1) {
    return launch_subsets_best(boot_subset_args(B, P, e0), P.units, s0, s1, include, B.ebest.ptr, ctx->stream, ne);
  };
  auto fit = [&](int64_t r, const double* G, const double* g, const double* H, const double* h, double inv_yy) {
    r2[r] = boot_r2(p, G, g, H, h, inv_yy);
  };
  return boot_best_blocks(ctx, P, W, R, seed, first, p, nullptr, launch, fit, v, masks, found, info);
}

// lsspa_boot_groups_best_run: groups_best_kernel's replicates over the block's reduced problems, boot_groups_run's in
// everything before the enumeration, with the g groups as the players and the caller's masks in B.ebest
static_assert(BOOT_GROUPS_BEST_MAX_PER == (1ull << (GROUPS_BEST_CLASSES - 1)),
              "boot_groups_best_plan's bound on per is groups_best_kernel's size classes");
int boot_groups_best_run(lsspa_ctx* ctx, const int32_t* labels, int32_t g, int64_t R, uint64_t seed, int64_t first,
                         const double* w_train, const double* w_test, int64_t block, double* u, uint32_t* masks,
                         uint8_t* found, double* r2, double* r2_base, int32_t* info) {
  BootWork& B = ctx->boot;
  GroupLayout L;      // lsspa_groups_best's messages (groups_args)
  TRY(boot_layout(ctx, labels, g, "exact attribution over groups takes at most g = %d groups (%d given)", L));
  BootPlan P;
  BootWeights W;
  TRY(boot_begin(ctx, "lsspa_boot_groups_best_run",
                 boot_groups_best_plan(R, B.n[0], B.n[1], B.p, L.ng, L.gh, L.nb, L.ql, block, P), R, w_train, w_test,
                 W));
  BootGroupR2 both(B.p, L);
  auto launch = [&](int e0, int ne, uint64_t s0, uint64_t s1) {
    return launch_groups_best(boot_group_args(B, P, L, e0), L.gid, P.units, s0, s1, B.ebest.ptr, ctx->stream, ne);
  };
  auto fit = [&](int64_t r, const double* G, const double* gv, const double* H, const double* h, double inv_yy) {
    both(G, gv, H, h, inv_yy, r2[r], r2_base[r]);
  };
  return boot_best_blocks(ctx, P, W, R, seed, first, L.ng, L.tab, launch, fit, u, masks, found, info);
}


}  // namespace

extern "C" {

int lsspa_debug_boot_plan(int64_t R, int64_t N, int64_t M, int32_t p, int64_t block, int64_t* plan15) try {
  if (!plan15) return LSSPA_ERR_ARG;
  BootPlan P;
  if (boot_plan(R, N, M, p, block, P)) return LSSPA_ERR_ARG;
  boot_plan15(P, plan15);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_NOMEM;
}

int lsspa_boot_load(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* y_train, int64_t N,
                    const void* X_test, int64_t ld_test, const void* y_test, int64_t M, int32_t p, double reg,
                    int32_t dtype, int32_t location) try {
  if (!ctx) return LSSPA_ERR_ARG;
  char msg[200];
  if (p > SUBSETS_MAX_P) {
    snprintf(msg, sizeof msg, "the bootstrap of the exact attribution takes at most p = %d features (%d given)",
             SUBSETS_MAX_P, (int)p);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  BootPlan P;
  if (const char* why = boot_plan(1, N, M, p, 0, P)) {
    snprintf(msg, sizeof msg, "lsspa_boot_load: %s", why);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  return boot_load_rows(ctx, P, "lsspa_boot_load", X_train, ld_train, y_train, N, X_test, ld_test, y_test, M, p, reg,
                        dtype, location);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_boot_groups_load(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* y_train, int64_t N,
                           const void* X_test, int64_t ld_test, const void* y_test, int64_t M, int32_t p, double reg,
                           int32_t dtype, int32_t location) try {
  if (!ctx) return LSSPA_ERR_ARG;
  char msg[200];
  if (p > GROUPS_MAX_P) {
    snprintf(msg, sizeof msg, "the bootstrap over groups of columns takes at most p = %d columns (%d given)",
             GROUPS_MAX_P, (int)p);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  BootPlan P;      // the rows' layout does not depend on the groups: the columns as one group
  if (const char* why = boot_groups_plan(1, N, M, p, 1, 1, 0, 0, 0, P)) {
    snprintf(msg, sizeof msg, "lsspa_boot_groups_load: %s", why);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  return boot_load_rows(ctx, P, "lsspa_boot_groups_load", X_train, ld_train, y_train, N, X_test, ld_test, y_test, M, p,
                        reg, dtype, location);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_boot_free(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->boot.release();
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_boot_run(lsspa_ctx* ctx, int64_t R, uint64_t seed, int64_t first, const double* w_train,
                   const double* w_test, int64_t block, double* phi, double* r2, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(boot_need_loaded(ctx));
  if (!phi || !r2 || !info || first < 0) return ctx->fail(LSSPA_ERR_ARG, "lsspa_boot_run: phi / r2 / info NULL or first < 0");
  return boot_subsets_run(ctx, "lsspa_boot_run", R, seed, first, w_train, w_test, block, phi, nullptr, r2, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_boot_interactions_run(lsspa_ctx* ctx, int64_t R, uint64_t seed, int64_t first, const double* w_train,
                                const double* w_test, int64_t block, double* phi, double* inter, double* r2,
                                int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(boot_need_loaded(ctx));
  if (!phi || !inter || !r2 || !info || first < 0)
    return ctx->fail(LSSPA_ERR_ARG, "lsspa_boot_interactions_run: phi / inter / r2 / info NULL or first < 0");
  return boot_subsets_run(ctx, "lsspa_boot_interactions_run", R, seed, first, w_train, w_test, block, phi, inter, r2,
                          info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_boot_inter_plan(int64_t R, int64_t N, int64_t M, int32_t p, int64_t block, int64_t* plan15) try {
  if (!plan15) return LSSPA_ERR_ARG;
  BootPlan P;
  if (boot_inter_plan(R, N, M, p, block, P)) return LSSPA_ERR_ARG;
  boot_plan15(P, plan15);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_NOMEM;
}

int lsspa_debug_boot_groups_plan(int64_t R, int64_t N, int64_t M, const int32_t* labels, int32_t p, int32_t g,
                                 int64_t block, int64_t* plan15) try {
  if (!plan15 || !labels || p < 1 || p > GROUPS_MAX_P) return LSSPA_ERR_ARG;
  GroupLayout L;
  if (groups_layout(labels, p, g, L)) return LSSPA_ERR_ARG;
  BootPlan P;
  if (boot_groups_plan(R, N, M, p, L.ng, L.gh, L.nb, L.ql, block, P)) return LSSPA_ERR_ARG;
  boot_plan15(P, plan15);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_NOMEM;
}

int lsspa_debug_boot_groups_inter_plan(int64_t R, int64_t N, int64_t M, const int32_t* labels, int32_t p, int32_t g,
                                       int64_t block, int64_t* plan15) try {
  if (!plan15 || !labels || p < 1 || p > GROUPS_MAX_P) return LSSPA_ERR_ARG;
  GroupLayout L;
  if (groups_layout(labels, p, g, L)) return LSSPA_ERR_ARG;
  BootPlan P;
  if (boot_groups_inter_plan(R, N, M, p, L.ng, L.gh, L.nb, L.ql, block, P)) return LSSPA_ERR_ARG;
  boot_plan15(P, plan15);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_NOMEM;
}

int lsspa_boot_groups_run(lsspa_ctx* ctx, const int32_t* labels, int32_t g, int64_t R, uint64_t seed, int64_t first,
                          const double* w_train, const double* w_test, int64_t block, double* phi, double* r2,
                          double* r2_base, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(boot_need_loaded(ctx));
  if (!labels || !phi || !r2 || !r2_base || !info || first < 0)
    return ctx->fail(LSSPA_ERR_ARG, "lsspa_boot_groups_run: labels / phi / r2 / r2_base / info NULL or first < 0");
  return boot_groups_run(ctx, "lsspa_boot_groups_run", labels, g, R, seed, first, w_train, w_test, block, phi, nullptr,
                         r2, r2_base, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_boot_groups_interactions_run(lsspa_ctx* ctx, const int32_t* labels, int32_t g, int64_t R, uint64_t seed,
                                       int64_t first, const double* w_train, const double* w_test, int64_t block,
                                       double* phi, double* inter, double* r2, double* r2_base, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(boot_need_loaded(ctx));
  if (!labels || !phi || !inter || !r2 || !r2_base || !info || first < 0)
    return ctx->fail(LSSPA_ERR_ARG,
                     "lsspa_boot_groups_interactions_run: labels / phi / inter / r2 / r2_base / info NULL or first < 0");
  return boot_groups_run(ctx, "lsspa_boot_groups_interactions_run", labels, g, R, seed, first, w_train, w_test, block,
                         phi, inter, r2, r2_base, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_boot_best_run(lsspa_ctx* ctx, int64_t R, uint64_t seed, int64_t first, const double* w_train,
                        const double* w_test, int64_t block, uint32_t include, double* v, uint32_t* masks,
                        uint8_t* found, double* r2, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(boot_need_loaded(ctx));
  if (!v || !masks || !found || !r2 || !info || first < 0)
    return ctx->fail(LSSPA_ERR_ARG, "lsspa_boot_best_run: v / masks / found / r2 / info NULL or first < 0");
  return boot_best_run(ctx, R, seed, first, w_train, w_test, block, include, v, masks, found, r2, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_boot_best_plan(int64_t R, int64_t N, int64_t M, int32_t p, int64_t block, int64_t* plan15) try {
  if (!plan15) return LSSPA_ERR_ARG;
  BootPlan P;
  if (boot_best_plan(R, N, M, p, block, P)) return LSSPA_ERR_ARG;
  boot_plan15(P, plan15);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_NOMEM;
}

int lsspa_boot_groups_best_run(lsspa_ctx* ctx, const int32_t* labels, int32_t g, int64_t R, uint64_t seed, int64_t first,
                               const double* w_train, const double* w_test, int64_t block, double* u, uint32_t* masks,
                               uint8_t* found, double* r2, double* r2_base, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(boot_need_loaded(ctx));
  if (!labels || !u || !masks || !found || !r2 || !r2_base || !info || first < 0)
    return ctx->fail(LSSPA_ERR_ARG,
                     "lsspa_boot_groups_best_run: labels / u / masks / found / r2 / r2_base / info NULL or first < 0");
  return boot_groups_best_run(ctx, labels, g, R, seed, first, w_train, w_test, block, u, masks, found, r2, r2_base,
                              info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_boot_groups_best_plan(int64_t R, int64_t N, int64_t M, const int32_t* labels, int32_t p, int32_t g,
                                      int64_t block, int64_t* plan15) try {
  if (!plan15 || !labels || p < 1 || p > GROUPS_MAX_P) return LSSPA_ERR_ARG;
  GroupLayout L;
  if (groups_layout(labels, p, g, L)) return LSSPA_ERR_ARG;
  BootPlan P;
  if (boot_groups_best_plan(R, N, M, p, L.ng, L.gh, L.nb, L.ql, block, P)) return LSSPA_ERR_ARG;
  boot_plan15(P, plan15);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_NOMEM;
}

int lsspa_boot_timing(const lsspa_ctx* ctx, double* counts_ms, double* gram_ms, double* enum_ms) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (counts_ms) *counts_ms = ctx->boot.ms[0];
  if (gram_ms) *gram_ms = ctx->boot.ms[1];
  if (enum_ms) *enum_ms = ctx->boot.ms[2];
  return LSSPA_OK;
} catch (...) {
  return abi_caught(const_cast<lsspa_ctx*>(ctx));
}

int lsspa_boot_debug_counts(lsspa_ctx* ctx, uint64_t seed, uint64_t r, int32_t side, uint32_t* out) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(boot_need_loaded(ctx));
  if (!out || side < 0 || side > 1) return ctx->fail(LSSPA_ERR_ARG, "lsspa_boot_debug_counts: out NULL or side not 0 / 1");
  HIPCHK(hipSetDevice(ctx->device));
  BootWork& B = ctx->boot;
  const int64_t n = B.n[side];
  TRY(dev_alloc(ctx, B.cnt(side), (size_t)n));
  HIPCHK(launch_boot_counts(seed, r, side, n, 1, B.cnt(side).ptr, ctx->stream));
  HIPCHK(hipMemcpyAsync(out, B.cnt(side).ptr, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_boot_debug_grams(lsspa_ctx* ctx, int64_t R, const double* w_train, const double* w_test, double* S_train,
                           double* S_test, double* wsum) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(boot_need_loaded(ctx));
  BootWork& B = ctx->boot;
  BootPlan P;
  BootWeights W;
  TRY(boot_begin(ctx, "lsspa_boot_debug_grams", boot_rows_plan(B, R, 0, P), R, w_train, w_test, W));
  W.counts[0] = W.counts[1] = false;     // a side without weights gets ones, not counts
  TRY(boot_alloc_block(ctx, P, W.counts, false));
  const size_t cc = (size_t)(B.p + 1) * (B.p + 1);
  for (int64_t b0 = 0; b0 < R; b0 += P.block) {
    const int nb = (int)std::min<int64_t>(P.block, R - b0);
    TRY(boot_block_sums(ctx, P, W.w_host, true, 0, 0, b0, nb, nullptr));
    if (S_train)
      HIPCHK(hipMemcpyAsync(S_train + b0 * cc, B.S0.ptr, sizeof(double) * nb * cc, hipMemcpyDeviceToHost, ctx->stream));
    if (S_test)
      HIPCHK(hipMemcpyAsync(S_test + b0 * cc, B.S1.ptr, sizeof(double) * nb * cc, hipMemcpyDeviceToHost, ctx->stream));
    if (wsum) HIPCHK(hipMemcpyAsync(wsum + b0, B.wsum.ptr, sizeof(double) * nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

}  // extern "C"

// ---- K-fold cross-validation (k_cv.hip, the CV kernels of k_subsets.hip) ---------------------------------------------
// lsspa_cv_load packs the rows once, forms the K per-fold Grams by the bootstrap's weighted Gram pass with indicator
// weights written on the device, and finalises the K fold problems into the replicate layout.  lsspa_cv_shapley runs the
// REPS enumeration over them, cut into launches as the one-problem call cuts a problem (the cut shows in the bits);
// lsspa_cv_best runs subsets_cv_best_kernel.
namespace {

int cv_need_loaded(lsspa_ctx* ctx) {
  if (!ctx->cv.loaded) return ctx->fail(LSSPA_ERR_STATE, "no cross-validation data loaded (lsspa_cv_load comes first)");
  return LSSPA_OK;
}

// k_subsets.hip's view of the fold problems from e0 on; info: the [K] words the call reports into
SubsetArgs cv_subset_args(const CvWork& W, int e0, int32_t* info) {
  SubsetArgs a{};
  a.p = W.p;
  a.q = subsets_low_features(W.p);
  a.w = W.w.ptr;
  rep_view(a, W.p, e0, W.G.ptr, W.g.ptr, W.H.ptr, W.h.ptr, W.inv_yy.ptr, info);
  return a;
}

// v [n] and, unless NULL, v_fold [n][K] of the host masks by subsets_cv_debug_kernel; the pivots' verdicts go to
// W.dinfo, which nobody reads: a value is what came out
int cv_values(lsspa_ctx* ctx, const uint64_t* masks, int64_t n, double* v, double* v_fold) {
  CvWork& W = ctx->cv;
  const int K = W.K;
  TRY(dev_alloc(ctx, W.masks, (size_t)n));
  TRY(dev_alloc(ctx, W.vals, (size_t)n * (K + 1)));
  TRY(dev_alloc(ctx, W.dinfo, CV_MAX_FOLDS));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpy(W.masks.ptr, masks, sizeof(uint64_t) * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(W.dinfo.ptr, 0, sizeof(int32_t) * CV_MAX_FOLDS, ctx->stream));
  SubsetArgs a = cv_subset_args(W, 0, W.dinfo.ptr);
  a.per = 1;
  HIPCHK(launch_subsets_cv_debug(a, K, W.masks.ptr, n, W.vals.ptr, v_fold ? W.vals.ptr + n : nullptr, ctx->stream));
  HIPCHK(hipMemcpyAsync(v, W.vals.ptr, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
  if (v_fold)
    HIPCHK(hipMemcpyAsync(v_fold, W.vals.ptr + n, sizeof(double) * n * K, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return LSSPA_OK;
}

// The enumeration of n replicate problems, `reps` of them a launch, on the cut of one problem: per set of replicates the
// partial table part [reps][units][cols] cleared, the kernels' view of the set's first replicate (view(e0): everything
// but per and part), the timed launches -- launch(a, s0, s1, ne): steps s0 .. s1 - 1 of every unit for the ne
// replicates behind a -- and the tables' column sums into out + e0 cols.  lsspa_cv_shapley, lsspa_cv_groups_shapley and
// a block of the ridge path; the bootstrap's block loop (boot_run_blocks) has the same inner loop without the events
// -- it times a block's whole enumeration -- and keeps its own.
template <typename View, typename Launch>
int rep_enumerate(lsspa_ctx* ctx, LaunchTimer& t, const EnumCut& c, int n, int reps, int cols, double* part, double* out,
                  View&& view, Launch&& launch) {
  hipStream_t st = ctx->stream;
  for (int e0 = 0; e0 < n; e0 += reps) {
    const int ne = std::min(reps, n - e0);
    HIPCHK(hipMemsetAsync(part, 0, sizeof(double) * (size_t)ne * c.units * cols, st));
    auto a = view(e0);
    a.per = c.per;
    a.part = part;
    TRY(t.run(ctx, c, [&](uint64_t s0, uint64_t s1) { return launch(a, s0, s1, ne); }));
    HIPCHK(launch_subsets_reduce(part, (int64_t)c.units, cols, out + (size_t)e0 * cols, st, ne));
  }
  return LSSPA_OK;
}

// The tail of the four CV selection calls: v_fold [n][K] is NaN but for the entries e with listed(e) -- the winners, the
// lists' valid ranks -- whose masks go through values(masks, n, v, v_fold), the kernel's own fold-step (cv_values, or
// cv_group_values on a layout)
template <typename Values, typename Listed>
int cv_fold_backfill(Values&& values, const uint32_t* masks, size_t n, Listed&& listed, int K, double* v_fold) {
  std::fill(v_fold, v_fold + n * K, std::nan(""));
  std::vector<uint64_t> m;
  std::vector<size_t> at;
  for (size_t e = 0; e < n; ++e)
    if (listed(e)) {
      at.push_back(e);
      m.push_back(masks[e]);
    }
  if (m.empty()) return LSSPA_OK;
  std::vector<double> v(m.size()), vf(m.size() * K);
  TRY(values(m.data(), (int64_t)m.size(), v.data(), vf.data()));
  for (size_t i = 0; i < m.size(); ++i) std::copy(&vf[i * K], &vf[i * K] + K, v_fold + at[i] * K);
  return LSSPA_OK;
}

// y [n] (host memory, dtype LSSPA_F64 / LSSPA_F32) has no entry that is not zero
bool host_all_zero(const void* y, int64_t n, int32_t dtype) {
  bool any = false;
  for (int64_t i = 0; i < n && !any; ++i)
    any = dtype == LSSPA_F32 ? ((const float*)y)[i] != 0.f : ((const double*)y)[i] != 0.0;
  return !any;
}

// max_p: SUBSETS_MAX_P (lsspa_cv_load) or GROUPS_MAX_P (lsspa_cv_groups_load); `name` is the entry point's
int cv_load(lsspa_ctx* ctx, const char* name, int max_p, const void* X, int64_t ld, const void* y, int64_t N, int32_t p,
            const int32_t* fold_ids, int32_t K, double reg, int32_t dtype, int32_t location) {
  char msg[240];
  if (p > max_p) {
    snprintf(msg, sizeof msg, "cross-validation enumerates feature subsets and takes at most p = %d features (%d given)",
             max_p, (int)p);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  if (K < 2 || K > CV_MAX_FOLDS) {
    snprintf(msg, sizeof msg, "cross-validation takes 2 .. %d folds (%d given)", CV_MAX_FOLDS, (int)K);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  if (!X || !y || !fold_ids || p < 1 || ld < p || !std::isfinite(reg) || (dtype != LSSPA_F64 && dtype != LSSPA_F32) ||
      (location != LSSPA_HOST && location != LSSPA_DEVICE))
  {
    snprintf(msg, sizeof msg, "%s: NULL array, p < 1, ld < p, reg not finite, or bad dtype / location", name);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  BootPlan P;      // the rows' layout and the Gram pass depend on N and p alone; beyond 32 columns: the columns as one group
  if (const char* why = p <= SUBSETS_MAX_P ? boot_plan(K, N, N, p, 0, P) : boot_groups_plan(K, N, N, p, 1, 1, 0, 0, 0, P)) {
    snprintf(msg, sizeof msg, "%s: %s", name, why);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  int32_t nf[CV_MAX_FOLDS] = {0};
  if (cv_count_folds(fold_ids, N, K, nf, msg, sizeof msg)) return ctx->fail(LSSPA_ERR_ARG, msg);
  // (rows on the device: the pooled sum is looked at after the Gram pass)
  if (location == LSSPA_HOST && host_all_zero(y, N, dtype))
    return ctx->fail(LSSPA_ERR_ARG, "y is identically zero (sum y^2 = 0): the cross-validated R^2 is not defined");
  HIPCHK(hipSetDevice(ctx->device));
  CvWork& W = ctx->cv;
  W.loaded = false;
  hipStream_t st = ctx->stream;
  const size_t c = (size_t)p + 1, pp = (size_t)p * p;
  TRY(dev_alloc(ctx, W.Z, (size_t)N * P.ldz));
  TRY(dev_alloc(ctx, W.fid, (size_t)N));
  TRY(dev_alloc(ctx, W.nf, CV_MAX_FOLDS));
  TRY(dev_alloc(ctx, W.wt, (size_t)K * N));
  TRY(dev_alloc(ctx, W.gpart, (size_t)P.slices[0] * K * P.pairs * 256));
  TRY(dev_alloc(ctx, W.S, (size_t)K * c * c));
  TRY(dev_alloc(ctx, W.G, (size_t)K * pp));
  TRY(dev_alloc(ctx, W.H, (size_t)K * pp));
  TRY(dev_alloc(ctx, W.g, (size_t)K * p));
  TRY(dev_alloc(ctx, W.h, (size_t)K * p));
  TRY(dev_alloc(ctx, W.inv_yy, CV_MAX_FOLDS));
  TRY(dev_alloc(ctx, W.info, CV_MAX_FOLDS));
  TRY(dev_alloc(ctx, W.w, EXACT_W_ROWS * (EXACT_MAX_PLAYERS + 1)));
  TRY(load_rows(ctx, W.stage_x, W.stage_y, X, ld, y, N, p, dtype, location,
                [&](const void* sx, const void* sy, int64_t nr, int64_t r0) {
                  return launch_boot_pack(sx, ld, sy, nr, p, dtype == LSSPA_F32, W.Z.ptr, P.ldz, r0, st);
                }));
  double w[EXACT_W_ROWS * (EXACT_MAX_PLAYERS + 1)] = {0.0};
  if (p <= SUBSETS_MAX_P) exact_weight_table(p, w);    // the column calls' weights; they refuse a wider load
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipMemcpy(W.w.ptr, w, sizeof w, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(W.fid.ptr, fold_ids, sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(W.nf.ptr, nf, sizeof nf, hipMemcpyHostToDevice));
  std::vector<hipEvent_t> ev(2, nullptr);
  Events guard{ev};
  for (hipEvent_t& e : ev) HIPCHK(hipEventCreate(&e));
  HIPCHK(hipEventRecord(ev[0], st));
  HIPCHK(launch_cv_weights(W.fid.ptr, N, K, W.wt.ptr, st));
  HIPCHK(launch_boot_gram(P, 0, W.Z.ptr, N, nullptr, W.wt.ptr, K, W.gpart.ptr, st));
  HIPCHK(launch_boot_reduce(P, 0, W.gpart.ptr, p, K, W.S.ptr, st));
  HIPCHK(launch_cv_finalize(W.S.ptr, W.nf.ptr, N, p, K, reg, W.G.ptr, W.g.ptr, W.H.ptr, W.h.ptr, W.inv_yy.ptr, st));
  HIPCHK(hipEventRecord(ev[1], st));
  W.Gh.resize(K * pp);
  W.Hh.resize(K * pp);
  W.gh.resize((size_t)K * p);
  W.hh.resize((size_t)K * p);
  W.yh.resize(K);
  HIPCHK(hipMemcpyAsync(W.Gh.data(), W.G.ptr, sizeof(double) * K * pp, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(W.Hh.data(), W.H.ptr, sizeof(double) * K * pp, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(W.gh.data(), W.g.ptr, sizeof(double) * K * p, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(W.hh.data(), W.h.ptr, sizeof(double) * K * p, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(W.yh.data(), W.inv_yy.ptr, sizeof(double) * K, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
  W.gram_ms = ms;
  W.enum_ms = W.max_launch_ms = 0.0;
  W.launches = 0;
  dev_free(W.stage_x);
  dev_free(W.stage_y);
  dev_free(W.wt);
  dev_free(W.gpart);
  if (!(W.yh[0] > 0.0) || !std::isfinite(W.yh[0]))
    return ctx->fail(LSSPA_ERR_ARG, "y is identically zero (sum y^2 = 0): the cross-validated R^2 is not defined");
  W.p = p;
  W.K = K;
  W.n = N;
  W.loaded = true;
  return LSSPA_OK;
}

int cv_shapley(lsspa_ctx* ctx, double* phi, double* phi_fold, double* r2_fold, int32_t* info) {
  CvWork& W = ctx->cv;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int p = W.p, K = W.K, cols = p + 1;
  // a fold's launches are the one-problem call's (the cut of `per` shows in the bits); as many folds share a launch as
  // its bound on the subsets of a launch leaves
  const EnumCut c(p);
  const uint64_t room = SUBSETS_PER_LAUNCH / (c.units * c.launch_steps());
  const int ereps = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)K, room));
  TRY(dev_alloc(ctx, W.part, (size_t)ereps * c.units * cols));
  TRY(dev_alloc(ctx, W.out, (size_t)K * cols));
  TRY(dev_alloc(ctx, W.phi, (size_t)(K + 1) * p));
  HIPCHK(hipMemsetAsync(W.info.ptr, 0, sizeof(int32_t) * CV_MAX_FOLDS, st));
  LaunchTimer t;
  TRY(rep_enumerate(ctx, t, c, K, ereps, cols, W.part.ptr, W.out.ptr,
                    [&](int e0) { return cv_subset_args(W, e0, W.info.ptr); },
                    [&](const SubsetArgs& a, uint64_t s0, uint64_t s1, int ne) {
                      return launch_subsets_enum(a, c.units, s0, s1, false, st, ne);
                    }));
  HIPCHK(launch_cv_foldsum(W.out.ptr, p, K, W.phi.ptr, W.phi.ptr + (size_t)K * p, st));
  HIPCHK(hipMemcpyAsync(phi_fold, W.phi.ptr, sizeof(double) * K * p, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(phi, W.phi.ptr + (size_t)K * p, sizeof(double) * p, hipMemcpyDeviceToHost, st));
  TRY(enum_finish(ctx, W, t, K, info));
  // each fold's share of the R^2 of the full model: the value of the full mask, fold by fold
  const uint64_t full = (1ull << p) - 1ull;      // p <= 32
  double v = 0.0;
  return cv_values(ctx, &full, 1, &v, r2_fold);
}

// lsspa_cv_best: best_run on the fold problems.  A step of a unit evaluates K fold problems, so a launch takes 1 / K of
// the steps the one-problem call gives it (EnumCut's K; steps > 0: the test hook)
int cv_best(lsspa_ctx* ctx, uint32_t include, int64_t steps, double* v, uint32_t* masks, uint8_t* found,
            double* v_fold, int32_t* info) {
  CvWork& W = ctx->cv;
  const int p = W.p, K = W.K;
  if (p < 32 && (include >> p) != 0u) return ctx->fail(LSSPA_ERR_ARG, "include names a feature beyond p");
  if (steps < 0) return ctx->fail(LSSPA_ERR_ARG, "lsspa_cv_best: steps must be >= 0");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemsetAsync(W.info.ptr, 0, sizeof(int32_t) * CV_MAX_FOLDS, ctx->stream));
  const EnumCut c(p, K, (uint64_t)steps);
  SubsetArgs a = cv_subset_args(W, 0, W.info.ptr);
  a.per = c.per;
  auto launch = [&](uint64_t s0, uint64_t s1) {
    a.part = W.part.ptr;
    return launch_subsets_cv_best(a, K, c.units, s0, s1, include, W.best.ptr, ctx->stream);
  };
  TRY(best_run(ctx, W, c, p, K, launch, v, masks, found, info));
  auto values = [&](const uint64_t* m, int64_t n, double* mv, double* mf) { return cv_values(ctx, m, n, mv, mf); };
  return cv_fold_backfill(values, masks, (size_t)p + 1, [&](size_t k) { return found[k] != 0; }, K, v_fold);
}

// lsspa_cv_top: top_run on the fold problems, cv_best's cut; the table depends on p and T alone
int cv_top(lsspa_ctx* ctx, uint32_t include, int T, int64_t steps, double* v, uint32_t* masks, int32_t* count,
           double* v_fold, int32_t* info) {
  CvWork& W = ctx->cv;
  const int p = W.p, K = W.K;
  if (p < 32 && (include >> p) != 0u) return ctx->fail(LSSPA_ERR_ARG, "include names a feature beyond p");
  if (T < 1 || T > SUBSETS_TOP_MAX) {
    char msg[120];
    snprintf(msg, sizeof msg, "lsspa_cv_top keeps 1 .. %d subsets of every size (T = %d)", SUBSETS_TOP_MAX, T);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  if (steps < 0) return ctx->fail(LSSPA_ERR_ARG, "lsspa_cv_top: steps must be >= 0");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemsetAsync(W.info.ptr, 0, sizeof(int32_t) * CV_MAX_FOLDS, ctx->stream));
  const EnumCut c(p, K, (uint64_t)steps);
  SubsetArgs a = cv_subset_args(W, 0, W.info.ptr);
  a.per = c.per;
  auto launch = [&](uint32_t* tm, int32_t* tc, uint64_t s0, uint64_t s1) {
    a.part = W.part.ptr;
    return launch_subsets_cv_top(a, K, c.units, s0, s1, include, T, tm, tc, ctx->stream);
  };
  TRY(top_run(ctx, W, c, TopTable(c, p, a.q, T), K, launch, v, masks, count, info));
  auto values = [&](const uint64_t* m, int64_t n, double* mv, double* mf) { return cv_values(ctx, m, n, mv, mf); };
  return cv_fold_backfill(values, masks, (size_t)(p + 1) * T, [&](size_t e) { return (int)(e % T) < count[e / T]; }, K,
                          v_fold);
}

// ---- ... over groups of columns (lsspa_cv_groups_*; the CV kernels of k_groups.hip) ----
// The fold problems are the same store; the players are the g groups of the labels, the baseline (label -1) is in every
// model.  lsspa_cv_groups_shapley runs the REPS enumeration of k_groups.hip over the folds, cut as lsspa_groups_shapley
// cuts one problem; lsspa_cv_groups_best runs groups_cv_best_kernel, lsspa_cv_groups_top groups_cv_top_kernel.

// the column calls after a grouped load of more columns than they enumerate
int cv_need_columns(lsspa_ctx* ctx, const char* name) {
  if (ctx->cv.p > SUBSETS_MAX_P) {
    char msg[280];
    snprintf(msg, sizeof msg, "%s enumerates feature subsets and takes at most p = %d features (%d loaded by "
             "lsspa_cv_groups_load: lsspa_cv_groups_shapley and lsspa_cv_groups_best work on groups of them)", name,
             SUBSETS_MAX_P, ctx->cv.p);
    return ctx->fail(LSSPA_ERR_STATE, msg);
  }
  return LSSPA_OK;
}

// labels / g against the loaded columns: lsspa_groups_shapley's limits and messages (groups_args)
int cv_layout(lsspa_ctx* ctx, const int32_t* labels, int32_t g, GroupLayout& L) {
  char msg[200];
  if (g > GROUPS_MAX_G) {
    snprintf(msg, sizeof msg, "exact attribution over groups takes at most g = %d groups (%d given)", GROUPS_MAX_G,
             (int)g);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  if (const char* why = groups_layout(labels, ctx->cv.p, g, L)) {
    snprintf(msg, sizeof msg, "group labels: %s", why);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  return LSSPA_OK;
}

// the weights of L.ng players and the layout table, for the launches of one call
int cv_groups_upload(lsspa_ctx* ctx, const GroupLayout& L) {
  CvWork& W = ctx->cv;
  constexpr int WR = EXACT_MAX_PLAYERS + 1;
  double w[EXACT_W_ROWS * WR];
  exact_weight_table(L.ng, w);
  TRY(dev_alloc(ctx, W.gw, EXACT_W_ROWS * WR));
  TRY(dev_alloc(ctx, W.tab, GROUPS_TAB_LEN));
  HIPCHK(hipStreamSynchronize(ctx->stream));   // a previous call may still read them; the copies are from host frames
  HIPCHK(hipMemcpy(W.gw.ptr, w, sizeof w, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(W.tab.ptr, L.tab, GROUPS_TAB_LEN * sizeof(int32_t), hipMemcpyHostToDevice));
  return LSSPA_OK;
}

// k_groups.hip's view of the fold problems from e0 on, over the layout L; info: the [K] words the call reports into
GroupArgs cv_group_args(const CvWork& W, const GroupLayout& L, int e0, int32_t* info) {
  GroupArgs a{};
  set_layout(a, L);
  a.w = W.gw.ptr;
  a.tab = W.tab.ptr;
  rep_view(a, W.p, e0, W.G.ptr, W.g.ptr, W.H.ptr, W.h.ptr, W.inv_yy.ptr, info);
  return a;
}

// u [n] and, unless NULL, u_fold [n][K] of the host masks (bit k = group k, the caller's numbering) by
// groups_cv_debug_kernel, after cv_groups_upload; the pivots' verdicts go to W.dinfo, which nobody reads
int cv_group_values(lsspa_ctx* ctx, const GroupLayout& L, const uint64_t* masks, int64_t n, double* u, double* u_fold) {
  CvWork& W = ctx->cv;
  const int K = W.K;
  const std::vector<uint64_t> lay = layout_masks(L, masks, n);
  TRY(dev_alloc(ctx, W.masks, (size_t)n));
  TRY(dev_alloc(ctx, W.vals, (size_t)n * (K + 1)));
  TRY(dev_alloc(ctx, W.dinfo, CV_MAX_FOLDS));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpy(W.masks.ptr, lay.data(), sizeof(uint64_t) * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(W.dinfo.ptr, 0, sizeof(int32_t) * CV_MAX_FOLDS, ctx->stream));
  GroupArgs a = cv_group_args(W, L, 0, W.dinfo.ptr);
  a.per = 1;
  HIPCHK(launch_groups_cv_debug(a, K, W.masks.ptr, n, W.vals.ptr, u_fold ? W.vals.ptr + n : nullptr, ctx->stream));
  HIPCHK(hipMemcpyAsync(u, W.vals.ptr, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
  if (u_fold)
    HIPCHK(hipMemcpyAsync(u_fold, W.vals.ptr + n, sizeof(double) * n * K, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return LSSPA_OK;
}

int cv_groups_shapley(lsspa_ctx* ctx, const int32_t* labels, int32_t g, double* phi, double* phi_fold, double* r2_fold,
                      double* base_fold, int32_t* info) {
  CvWork& W = ctx->cv;
  GroupLayout L;
  TRY(cv_layout(ctx, labels, g, L));
  HIPCHK(hipSetDevice(ctx->device));
  TRY(cv_groups_upload(ctx, L));
  hipStream_t st = ctx->stream;
  const int K = W.K, ng = L.ng, cols = ng + 1;
  // a fold's launches are lsspa_groups_shapley's (the cut of `per` shows in the bits); as many folds share a launch as
  // its work bound and the 2^20 workgroups of a launch leave (boot_groups_plan's rule)
  const EnumCut c(L);
  const uint64_t room = std::min<uint64_t>(1ull << 20, groups_per_launch(L)) / (c.units * c.launch_steps());
  const int ereps = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)K, room));
  TRY(dev_alloc(ctx, W.part, (size_t)ereps * c.units * cols));
  TRY(dev_alloc(ctx, W.out, (size_t)K * cols));
  TRY(dev_alloc(ctx, W.phi, (size_t)(K + 1) * ng));
  HIPCHK(hipMemsetAsync(W.info.ptr, 0, sizeof(int32_t) * CV_MAX_FOLDS, st));
  LaunchTimer t;
  TRY(rep_enumerate(ctx, t, c, K, ereps, cols, W.part.ptr, W.out.ptr,
                    [&](int e0) { return cv_group_args(W, L, e0, W.info.ptr); },
                    [&](const GroupArgs& a, uint64_t s0, uint64_t s1, int ne) {
                      return launch_groups_enum(a, c.units, s0, s1, false, st, ne);
                    }));
  // a fold into label order as the bootstrap finishes a replicate, then the folds' sum in ascending order
  HIPCHK(launch_cv_groups_foldsum(W.out.ptr, ng, K, L.gid, W.phi.ptr, W.phi.ptr + (size_t)K * ng, st));
  HIPCHK(hipMemcpyAsync(phi_fold, W.phi.ptr, sizeof(double) * K * ng, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(phi, W.phi.ptr + (size_t)K * ng, sizeof(double) * ng, hipMemcpyDeviceToHost, st));
  TRY(enum_finish(ctx, W, t, K, info));
  // each fold's value of all groups and of the baseline alone, fold by fold
  const uint64_t both[2] = {ng < 64 ? (1ull << ng) - 1ull : ~0ull, 0ull};
  double u[2];
  std::vector<double> uf((size_t)2 * K);
  TRY(cv_group_values(ctx, L, both, 2, u, uf.data()));
  std::copy(uf.begin(), uf.begin() + K, r2_fold);
  std::copy(uf.begin() + K, uf.end(), base_fold);
  return LSSPA_OK;
}

// lsspa_cv_groups_best: best_run on the fold problems with the g groups as the players; cv_best's rule for the cut
int cv_groups_best(lsspa_ctx* ctx, const int32_t* labels, int32_t g, int64_t steps, double* u, uint32_t* masks,
                   uint8_t* found, double* u_fold, int32_t* info) {
  CvWork& W = ctx->cv;
  if (steps < 0) return ctx->fail(LSSPA_ERR_ARG, "lsspa_cv_groups_best: steps must be >= 0");
  GroupLayout L;
  TRY(cv_layout(ctx, labels, g, L));
  HIPCHK(hipSetDevice(ctx->device));
  TRY(cv_groups_upload(ctx, L));
  HIPCHK(hipMemsetAsync(W.info.ptr, 0, sizeof(int32_t) * CV_MAX_FOLDS, ctx->stream));
  const int K = W.K;
  const EnumCut c(L, K, (uint64_t)steps);
  GroupArgs a = cv_group_args(W, L, 0, W.info.ptr);
  a.per = c.per;
  auto launch = [&](uint64_t s0, uint64_t s1) {
    a.part = W.part.ptr;
    return launch_groups_cv_best(a, K, L.gid, c.units, s0, s1, W.best.ptr, ctx->stream);
  };
  TRY(best_run(ctx, W, c, L.ng, K, launch, u, masks, found, info));
  auto values = [&](const uint64_t* m, int64_t n, double* mv, double* mf) {
    return cv_group_values(ctx, L, m, n, mv, mf);
  };
  return cv_fold_backfill(values, masks, (size_t)L.ng + 1, [&](size_t k) { return found[k] != 0; }, K, u_fold);
}

// lsspa_cv_groups_top: top_run on the fold problems, cv_groups_best's cut; the table depends on the layout and T alone
int cv_groups_top(lsspa_ctx* ctx, const int32_t* labels, int32_t g, int T, int64_t steps, double* u, uint32_t* masks,
                  int32_t* count, double* u_fold, int32_t* info) {
  CvWork& W = ctx->cv;
  GroupLayout L;
  TRY(cv_layout(ctx, labels, g, L));
  if (T < 1 || T > GROUPS_TOP_MAX) {
    char msg[120];
    snprintf(msg, sizeof msg, "lsspa_cv_groups_top keeps 1 .. %d subsets of every size (T = %d)", GROUPS_TOP_MAX, T);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  if (steps < 0) return ctx->fail(LSSPA_ERR_ARG, "lsspa_cv_groups_top: steps must be >= 0");
  HIPCHK(hipSetDevice(ctx->device));
  TRY(cv_groups_upload(ctx, L));
  HIPCHK(hipMemsetAsync(W.info.ptr, 0, sizeof(int32_t) * CV_MAX_FOLDS, ctx->stream));
  const int K = W.K;
  const EnumCut c(L, K, (uint64_t)steps);
  GroupArgs a = cv_group_args(W, L, 0, W.info.ptr);
  a.per = c.per;
  auto launch = [&](uint32_t* tm, int32_t* tc, uint64_t s0, uint64_t s1) {
    a.part = W.part.ptr;
    return launch_groups_cv_top(a, K, L.gid, c.units, s0, s1, T, tm, tc, ctx->stream);
  };
  TRY(top_run(ctx, W, c, TopTable(c, L.ng, L.gl, T), K, launch, u, masks, count, info));
  auto values = [&](const uint64_t* m, int64_t n, double* mv, double* mf) {
    return cv_group_values(ctx, L, m, n, mv, mf);
  };
  return cv_fold_backfill(values, masks, (size_t)(L.ng + 1) * T, [&](size_t e) { return (int)(e % T) < count[e / T]; },
                          K, u_fold);
}

}  // namespace

extern "C" {

int lsspa_cv_groups_load(lsspa_ctx* ctx, const void* X, int64_t ld, const void* y, int64_t N, int32_t p,
                         const int32_t* fold_ids, int32_t K, double reg, int32_t dtype, int32_t location) try {
  if (!ctx) return LSSPA_ERR_ARG;
  return cv_load(ctx, "lsspa_cv_groups_load", GROUPS_MAX_P, X, ld, y, N, p, fold_ids, K, reg, dtype, location);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_cv_groups_shapley(lsspa_ctx* ctx, const int32_t* labels, int32_t g, double* phi, double* phi_fold,
                            double* r2_fold, double* base_fold, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(cv_need_loaded(ctx));
  if (!labels || !phi || !phi_fold || !r2_fold || !base_fold || !info)
    return ctx->fail(LSSPA_ERR_ARG, "lsspa_cv_groups_shapley: labels / phi / phi_fold / r2_fold / base_fold / info is NULL");
  return cv_groups_shapley(ctx, labels, g, phi, phi_fold, r2_fold, base_fold, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_cv_groups_best(lsspa_ctx* ctx, const int32_t* labels, int32_t g, int64_t steps, double* u, uint32_t* masks,
                         uint8_t* found, double* u_fold, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(cv_need_loaded(ctx));
  if (!labels || !u || !masks || !found || !u_fold || !info)
    return ctx->fail(LSSPA_ERR_ARG, "lsspa_cv_groups_best: labels / u / masks / found / u_fold / info is NULL");
  return cv_groups_best(ctx, labels, g, steps, u, masks, found, u_fold, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_cv_groups_top(lsspa_ctx* ctx, const int32_t* labels, int32_t g, int32_t T, int64_t steps, double* u,
                        uint32_t* masks, int32_t* count, double* u_fold, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(cv_need_loaded(ctx));
  if (!labels || !u || !masks || !count || !u_fold || !info)
    return ctx->fail(LSSPA_ERR_ARG, "lsspa_cv_groups_top: labels / u / masks / count / u_fold / info is NULL");
  return cv_groups_top(ctx, labels, g, T, steps, u, masks, count, u_fold, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_cv_groups_top_plan(const int32_t* labels, int32_t p, int32_t g, int32_t K, int32_t T,
                                   int64_t* plan) try {
  GroupLayout L;
  if (!plan || g > GROUPS_MAX_G || p > GROUPS_MAX_P || K < 2 || K > CV_MAX_FOLDS || T < 1 || T > GROUPS_TOP_MAX ||
      groups_layout(labels, p, g, L))
    return LSSPA_ERR_ARG;
  const EnumCut c(L, K);
  const TopTable tab(c, L.ng, L.gl, T);
  const int64_t out[12] = {L.gl, L.gh, L.ql, L.nb, (int64_t)c.units, (int64_t)c.per, (int64_t)c.launch_steps(),
                           (int64_t)c.launches, (int64_t)groups_cv_top_lds_bytes(), 256, tab.sizes, tab.bytes};
  std::copy(out, out + 12, plan);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_ARG;
}

int lsspa_debug_cv_group_values(lsspa_ctx* ctx, const int32_t* labels, int32_t g, const uint64_t* masks, int64_t n,
                                double* u, double* u_fold) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(cv_need_loaded(ctx));
  if (!labels || n < 0 || (n > 0 && (!masks || !u))) return ctx->fail(LSSPA_ERR_ARG, "labels / masks / u NULL or n < 0");
  GroupLayout L;
  TRY(cv_layout(ctx, labels, g, L));
  const uint64_t full = L.ng < 64 ? (1ull << L.ng) - 1ull : ~0ull;
  for (int64_t i = 0; i < n; ++i)
    if (masks[i] & ~full) return ctx->fail(LSSPA_ERR_ARG, "a mask names a group beyond g");
  if (n == 0) return LSSPA_OK;
  HIPCHK(hipSetDevice(ctx->device));
  TRY(cv_groups_upload(ctx, L));
  return cv_group_values(ctx, L, masks, n, u, u_fold);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_cv_groups_plan(const int32_t* labels, int32_t p, int32_t g, int32_t K, int64_t* plan) try {
  GroupLayout L;
  if (!plan || g > GROUPS_MAX_G || p > GROUPS_MAX_P || K < 2 || K > CV_MAX_FOLDS || groups_layout(labels, p, g, L))
    return LSSPA_ERR_ARG;
  const EnumCut c(L, K);
  const int64_t out[12] = {L.gl, L.gh, L.ql, L.nb, (int64_t)c.units, (int64_t)c.per, (int64_t)c.launch_steps(),
                           (int64_t)c.launches, (int64_t)groups_cv_lds_bytes(), 256, (int64_t)groups_best_lds_bytes(),
                           (int64_t)groups_per_launch(L)};
  std::copy(out, out + 12, plan);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_ARG;
}

int lsspa_cv_load(lsspa_ctx* ctx, const void* X, int64_t ld, const void* y, int64_t N, int32_t p,
                  const int32_t* fold_ids, int32_t K, double reg, int32_t dtype, int32_t location) try {
  if (!ctx) return LSSPA_ERR_ARG;
  return cv_load(ctx, "lsspa_cv_load", SUBSETS_MAX_P, X, ld, y, N, p, fold_ids, K, reg, dtype, location);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_cv_shapley(lsspa_ctx* ctx, double* phi, double* phi_fold, double* r2_fold, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(cv_need_loaded(ctx));
  TRY(cv_need_columns(ctx, "lsspa_cv_shapley"));
  if (!phi || !phi_fold || !r2_fold || !info)
    return ctx->fail(LSSPA_ERR_ARG, "lsspa_cv_shapley: phi / phi_fold / r2_fold / info is NULL");
  return cv_shapley(ctx, phi, phi_fold, r2_fold, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_cv_best(lsspa_ctx* ctx, uint32_t include, int64_t steps, double* v, uint32_t* masks, uint8_t* found,
                  double* v_fold, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(cv_need_loaded(ctx));
  TRY(cv_need_columns(ctx, "lsspa_cv_best"));
  if (!v || !masks || !found || !v_fold || !info)
    return ctx->fail(LSSPA_ERR_ARG, "lsspa_cv_best: v / masks / found / v_fold / info is NULL");
  return cv_best(ctx, include, steps, v, masks, found, v_fold, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_cv_top(lsspa_ctx* ctx, uint32_t include, int32_t T, int64_t steps, double* v, uint32_t* masks, int32_t* count,
                 double* v_fold, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(cv_need_loaded(ctx));
  TRY(cv_need_columns(ctx, "lsspa_cv_top"));
  if (!v || !masks || !count || !v_fold || !info)
    return ctx->fail(LSSPA_ERR_ARG, "lsspa_cv_top: v / masks / count / v_fold / info is NULL");
  return cv_top(ctx, include, T, steps, v, masks, count, v_fold, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_cv_timing(const lsspa_ctx* ctx, double* gram_ms, double* enum_ms, double* max_launch_ms,
                    int64_t* launches) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (gram_ms) *gram_ms = ctx->cv.gram_ms;
  if (enum_ms) *enum_ms = ctx->cv.enum_ms;
  if (max_launch_ms) *max_launch_ms = ctx->cv.max_launch_ms;
  if (launches) *launches = ctx->cv.launches;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(const_cast<lsspa_ctx*>(ctx));
}

int lsspa_cv_free(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->cv.release();
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_cv_get_problem(lsspa_ctx* ctx, int32_t f, double* G, double* g, double* H, double* h, double* inv_yy) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(cv_need_loaded(ctx));
  const CvWork& W = ctx->cv;
  if (f < 0 || f >= W.K) return ctx->fail(LSSPA_ERR_ARG, "lsspa_cv_get_problem: f must be 0 .. K - 1");
  const size_t p = (size_t)W.p, pp = p * p;
  if (G) std::copy(&W.Gh[f * pp], &W.Gh[f * pp] + pp, G);
  if (H) std::copy(&W.Hh[f * pp], &W.Hh[f * pp] + pp, H);
  if (g) std::copy(&W.gh[f * p], &W.gh[f * p] + p, g);
  if (h) std::copy(&W.hh[f * p], &W.hh[f * p] + p, h);
  if (inv_yy) *inv_yy = W.yh[f];
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_cv_values(lsspa_ctx* ctx, const uint64_t* masks, int64_t n, double* v, double* v_fold) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(cv_need_loaded(ctx));
  TRY(cv_need_columns(ctx, "lsspa_debug_cv_values"));
  if (n < 0 || (n > 0 && (!masks || !v))) return ctx->fail(LSSPA_ERR_ARG, "masks / v NULL or n < 0");
  const uint64_t full = (1ull << ctx->cv.p) - 1ull;     // p <= 32 here
  for (int64_t i = 0; i < n; ++i)
    if (masks[i] & ~full) return ctx->fail(LSSPA_ERR_ARG, "a mask names a feature beyond p");
  if (n == 0) return LSSPA_OK;
  HIPCHK(hipSetDevice(ctx->device));
  return cv_values(ctx, masks, n, v, v_fold);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_cv_plan(int32_t p, int32_t K, int64_t* plan) try {
  if (!plan || p < 1 || p > SUBSETS_MAX_P || K < 2 || K > CV_MAX_FOLDS) return LSSPA_ERR_ARG;
  const EnumCut c(p, K);
  const int64_t out[8] = {(int64_t)c.units, (int64_t)c.per, (int64_t)c.launch_steps(), (int64_t)c.launches,
                          (int64_t)subsets_cv_lds_bytes(), 64, 0, 0};
  std::copy(out, out + 8, plan);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_NOMEM;
}

int lsspa_debug_cv_top_plan(int32_t p, int32_t K, int32_t T, int64_t* plan) try {
  if (!plan || p < 1 || p > SUBSETS_MAX_P || K < 2 || K > CV_MAX_FOLDS || T < 1 || T > SUBSETS_TOP_MAX)
    return LSSPA_ERR_ARG;
  const EnumCut c(p, K);
  const TopTable tab(c, p, subsets_low_features(p), T);
  const int64_t out[8] = {(int64_t)c.units, (int64_t)c.per, (int64_t)c.launch_steps(), (int64_t)c.launches,
                          (int64_t)subsets_cv_top_lds_bytes(T), 64, tab.sizes, tab.bytes};
  std::copy(out, out + 8, plan);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_NOMEM;
}

}  // extern "C"

// ---- the ridge path of the K-fold CV attribution (lsspa_cv_path_*; the path kernels of k_cv.hip) ---------------------
// reg enters a fold problem only as + reg on the diagonal of G_f, and the load keeps the per-fold Grams S: L ridge values
// are L K fold problems written from S on the device (launch_cv_path_finalize) and enumerated as replicates of shared
// grids, a block of ridge values at a time.  A problem is cut into launches exactly as cv_shapley / cv_groups_shapley
// cut a fold (the cut of `per` shows in the bits) and a replicate's result does not depend on the replicates beside it,
// so row l has the bits of a load with reg = regs[l].  Everything the path writes is CvWork::Path's.
namespace {

constexpr size_t CV_PATH_BLOCK_BYTES = 64ull << 20;   // the problems of a block of ridge values stay inside this

struct CvPathPlan {
  EnumCut cut;                  // one problem's: that of cv_shapley / cv_groups_shapley
  uint64_t bound, room;         // subsets a launch takes over its units, steps and replicates; replicates that leaves
  int block, blocks, reps;      // ridge values a block; blocks of L values; replicates of a launch of a full block
  uint64_t launches;            // enumeration launches of the L values
  // at most `bound` subsets a launch; forced > 0: that many ridge values a block (test hook; cut to L)
  CvPathPlan(const EnumCut& c, uint64_t bound_, int p, int K, int L, int forced) : cut(c), bound(bound_) {
    room = std::max<uint64_t>(1, bound / (cut.units * cut.launch_steps()));
    const size_t problem = sizeof(double) * (2 * (size_t)p * p + 2 * (size_t)p + 1) * (size_t)K;
    block = forced > 0 ? forced : (int)std::max<size_t>(1, CV_PATH_BLOCK_BYTES / problem);
    block = std::min(block, L);
    blocks = (L + block - 1) / block;
    reps = (int)std::min<uint64_t>((uint64_t)block * K, room);
    launches = 0;
    for (int l0 = 0; l0 < L; l0 += block) {
      const uint64_t n = (uint64_t)std::min(block, L - l0) * K, r = std::min(n, room);
      launches += ((n + r - 1) / r) * cut.launches;
    }
  }
};
CvPathPlan cv_path_columns_plan(int p, int K, int L, int forced) {
  return CvPathPlan(EnumCut(p), SUBSETS_PER_LAUNCH, p, K, L, forced);
}
CvPathPlan cv_path_groups_plan(const GroupLayout& G, int K, int L, int forced) {
  return CvPathPlan(EnumCut(G), std::min<uint64_t>(1ull << 20, groups_per_launch(G)), G.p, K, L, forced);
}

// regs [L], L and block of both entry points
int cv_path_check(lsspa_ctx* ctx, const char* name, const double* regs, int32_t L, int32_t block) {
  char msg[200];
  if (L < 1 || L > CV_PATH_MAX_REGS) {
    snprintf(msg, sizeof msg, "%s takes 1 .. %d ridge values (L = %d)", name, CV_PATH_MAX_REGS, (int)L);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  if (block < 0) {
    snprintf(msg, sizeof msg, "%s: block must be >= 0", name);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  for (int l = 0; l < L; ++l)
    if (!std::isfinite(regs[l]) || regs[l] < 0.0) {
      snprintf(msg, sizeof msg, "%s: regs[%d] = %g: a ridge value must be finite and >= 0", name, l, regs[l]);
      return ctx->fail(LSSPA_ERR_ARG, msg);
    }
  return LSSPA_OK;
}

// a0 with the path's problems from replicate e0 on
template <typename Args>
Args cv_path_args(const CvWork::Path& Q, int p, const Args& a0, int e0) {
  Args a = a0;
  rep_view(a, p, e0, Q.G.ptr, Q.g.ptr, Q.H.ptr, Q.h.ptr, Q.inv_yy.ptr, Q.info.ptr);
  return a;
}

// One block: the problems of the nl ridge values regs (host) into W.path, their enumeration (rep_enumerate with the
// entry point's launch) and the tables' sums into Q.out [nl K][cols].  a0: the call's arguments but for the problems'
// pointers; t: the call's timer.
template <typename Args, typename Launch>
int cv_path_block(lsspa_ctx* ctx, const CvPathPlan& P, int cols, const double* regs, int nl, const Args& a0,
                  Launch&& launch, LaunchTimer& t) {
  CvWork& W = ctx->cv;
  CvWork::Path& Q = W.path;
  hipStream_t st = ctx->stream;
  const int p = W.p, K = W.K, n = nl * K;
  const size_t pp = (size_t)p * p;
  const int reps = (int)std::min<uint64_t>((uint64_t)n, P.room);
  TRY(dev_alloc(ctx, Q.regs, (size_t)nl));
  TRY(dev_alloc(ctx, Q.G, (size_t)n * pp));
  TRY(dev_alloc(ctx, Q.H, (size_t)n * pp));
  TRY(dev_alloc(ctx, Q.g, (size_t)n * p));
  TRY(dev_alloc(ctx, Q.h, (size_t)n * p));
  TRY(dev_alloc(ctx, Q.inv_yy, (size_t)n));
  TRY(dev_alloc(ctx, Q.info, (size_t)n));
  TRY(dev_alloc(ctx, Q.part, (size_t)reps * P.cut.units * cols));
  TRY(dev_alloc(ctx, Q.out, (size_t)n * cols));
  HIPCHK(hipStreamSynchronize(st));            // the copy is from the caller's array; a block before this one is done
  HIPCHK(hipMemcpy(Q.regs.ptr, regs, sizeof(double) * nl, hipMemcpyHostToDevice));
  HIPCHK(launch_cv_path_finalize(W.S.ptr, W.nf.ptr, Q.regs.ptr, nl, W.n, p, K, Q.G.ptr, Q.g.ptr, Q.H.ptr, Q.h.ptr,
                                 Q.inv_yy.ptr, st));
  HIPCHK(hipMemsetAsync(Q.info.ptr, 0, sizeof(int32_t) * n, st));
  return rep_enumerate(ctx, t, P.cut, n, reps, cols, Q.part.ptr, Q.out.ptr,
                       [&](int e0) { return cv_path_args(Q, p, a0, e0); }, launch);
}

int cv_path_shapley(lsspa_ctx* ctx, const double* regs, int L, int block, double* phi, double* phi_fold,
                    double* r2_fold, int32_t* info) {
  CvWork& W = ctx->cv;
  CvWork::Path& Q = W.path;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int p = W.p, K = W.K, cols = p + 1;
  const CvPathPlan P = cv_path_columns_plan(p, K, L, block);
  LaunchTimer t;
  const SubsetArgs a0 = cv_subset_args(W, 0, W.info.ptr);    // p, q, the weights and the pivot test
  const uint64_t full = (1ull << p) - 1ull;                   // p <= 32
  TRY(dev_alloc(ctx, Q.masks, 1));
  TRY(dev_alloc(ctx, Q.dinfo, CV_MAX_FOLDS));
  TRY(dev_alloc(ctx, Q.phi, (size_t)P.block * (K + 1) * p));
  TRY(dev_alloc(ctx, Q.vals, (size_t)P.block * (K + 1)));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipMemcpy(Q.masks.ptr, &full, sizeof full, hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(Q.dinfo.ptr, 0, sizeof(int32_t) * CV_MAX_FOLDS, st));
  for (int l0 = 0; l0 < L; l0 += P.block) {
    const int nl = std::min(P.block, L - l0);
    TRY(cv_path_block(ctx, P, cols, regs + l0, nl, a0,
                      [&](const SubsetArgs& a, uint64_t s0, uint64_t s1, int ne) {
                        return launch_subsets_enum(a, P.cut.units, s0, s1, false, st, ne);
                      },
                      t));
    double* fold = Q.phi.ptr;
    double* sum = Q.phi.ptr + (size_t)nl * K * p;
    HIPCHK(launch_cv_path_foldsum(Q.out.ptr, p, K, nl, fold, sum, st));
    // each fold's share of the R^2 of the full model, ridge value by ridge value: cv_values on the path's problems
    for (int i = 0; i < nl; ++i) {
      SubsetArgs a = cv_path_args(Q, p, a0, i * K);
      a.info = Q.dinfo.ptr;
      a.per = 1;
      double* v = Q.vals.ptr + (size_t)i * (K + 1);
      HIPCHK(launch_subsets_cv_debug(a, K, Q.masks.ptr, 1, v, v + 1, st));
    }
    HIPCHK(hipMemcpyAsync(phi_fold + (size_t)l0 * K * p, fold, sizeof(double) * nl * K * p, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(phi + (size_t)l0 * p, sum, sizeof(double) * nl * p, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(info + (size_t)l0 * K, Q.info.ptr, sizeof(int32_t) * nl * K, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpy2DAsync(r2_fold + (size_t)l0 * K, sizeof(double) * K, Q.vals.ptr + 1, sizeof(double) * (K + 1),
                            sizeof(double) * K, (size_t)nl, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  return keep_timing(ctx, W, t);
}

int cv_path_groups_shapley(lsspa_ctx* ctx, const int32_t* labels, int32_t g, const double* regs, int L, int block,
                           double* phi, double* phi_fold, double* r2_fold, double* base_fold, int32_t* info) {
  CvWork& W = ctx->cv;
  CvWork::Path& Q = W.path;
  GroupLayout G;
  TRY(cv_layout(ctx, labels, g, G));
  HIPCHK(hipSetDevice(ctx->device));
  TRY(cv_groups_upload(ctx, G));
  hipStream_t st = ctx->stream;
  const int K = W.K, ng = G.ng, cols = ng + 1;
  const CvPathPlan P = cv_path_groups_plan(G, K, L, block);
  LaunchTimer t;
  const GroupArgs a0 = cv_group_args(W, G, 0, W.info.ptr);   // the layout, the weights, the table and the pivot test
  // all groups and the baseline alone (the same mask in the layout's numbering and the caller's)
  const uint64_t both[2] = {ng < 64 ? (1ull << ng) - 1ull : ~0ull, 0ull};
  const size_t vs = 2 * (size_t)(K + 1);                      // a ridge value's values: u [2], u_fold [2][K]
  TRY(dev_alloc(ctx, Q.masks, 2));
  TRY(dev_alloc(ctx, Q.dinfo, CV_MAX_FOLDS));
  TRY(dev_alloc(ctx, Q.phi, (size_t)P.block * (K + 1) * ng));
  TRY(dev_alloc(ctx, Q.vals, (size_t)P.block * vs));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipMemcpy(Q.masks.ptr, both, sizeof both, hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(Q.dinfo.ptr, 0, sizeof(int32_t) * CV_MAX_FOLDS, st));
  for (int l0 = 0; l0 < L; l0 += P.block) {
    const int nl = std::min(P.block, L - l0);
    TRY(cv_path_block(ctx, P, cols, regs + l0, nl, a0,
                      [&](const GroupArgs& a, uint64_t s0, uint64_t s1, int ne) {
                        return launch_groups_enum(a, P.cut.units, s0, s1, false, st, ne);
                      },
                      t));
    double* fold = Q.phi.ptr;
    double* sum = Q.phi.ptr + (size_t)nl * K * ng;
    HIPCHK(launch_cv_path_groups_foldsum(Q.out.ptr, ng, K, nl, G.gid, fold, sum, st));
    for (int i = 0; i < nl; ++i) {
      GroupArgs a = cv_path_args(Q, W.p, a0, i * K);
      a.info = Q.dinfo.ptr;
      a.per = 1;
      double* u = Q.vals.ptr + (size_t)i * vs;
      HIPCHK(launch_groups_cv_debug(a, K, Q.masks.ptr, 2, u, u + 2, st));
    }
    HIPCHK(hipMemcpyAsync(phi_fold + (size_t)l0 * K * ng, fold, sizeof(double) * nl * K * ng, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(phi + (size_t)l0 * ng, sum, sizeof(double) * nl * ng, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(info + (size_t)l0 * K, Q.info.ptr, sizeof(int32_t) * nl * K, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpy2DAsync(r2_fold + (size_t)l0 * K, sizeof(double) * K, Q.vals.ptr + 2, sizeof(double) * vs,
                            sizeof(double) * K, (size_t)nl, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpy2DAsync(base_fold + (size_t)l0 * K, sizeof(double) * K, Q.vals.ptr + 2 + K, sizeof(double) * vs,
                            sizeof(double) * K, (size_t)nl, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  return keep_timing(ctx, W, t);
}

}  // namespace

extern "C" {

int lsspa_cv_path_shapley(lsspa_ctx* ctx, const double* regs, int32_t L, int32_t block, double* phi, double* phi_fold,
                          double* r2_fold, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(cv_need_loaded(ctx));
  TRY(cv_need_columns(ctx, "lsspa_cv_path_shapley"));
  if (!regs || !phi || !phi_fold || !r2_fold || !info)
    return ctx->fail(LSSPA_ERR_ARG, "lsspa_cv_path_shapley: regs / phi / phi_fold / r2_fold / info is NULL");
  TRY(cv_path_check(ctx, "lsspa_cv_path_shapley", regs, L, block));
  return cv_path_shapley(ctx, regs, L, block, phi, phi_fold, r2_fold, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_cv_path_groups_shapley(lsspa_ctx* ctx, const int32_t* labels, int32_t g, const double* regs, int32_t L,
                                 int32_t block, double* phi, double* phi_fold, double* r2_fold, double* base_fold,
                                 int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(cv_need_loaded(ctx));
  if (!labels || !regs || !phi || !phi_fold || !r2_fold || !base_fold || !info)
    return ctx->fail(LSSPA_ERR_ARG,
                     "lsspa_cv_path_groups_shapley: labels / regs / phi / phi_fold / r2_fold / base_fold / info is NULL");
  TRY(cv_path_check(ctx, "lsspa_cv_path_groups_shapley", regs, L, block));
  return cv_path_groups_shapley(ctx, labels, g, regs, L, block, phi, phi_fold, r2_fold, base_fold, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_cv_path_plan(int32_t p, int32_t K, int32_t L, int32_t block, int64_t* plan) try {
  if (!plan || p < 1 || p > SUBSETS_MAX_P || K < 2 || K > CV_MAX_FOLDS || L < 1 || L > CV_PATH_MAX_REGS || block < 0)
    return LSSPA_ERR_ARG;
  const CvPathPlan P = cv_path_columns_plan(p, K, L, block);
  const int64_t out[8] = {(int64_t)P.cut.units, (int64_t)P.cut.per, (int64_t)P.cut.launch_steps(), P.block, P.blocks,
                          P.reps, (int64_t)P.launches, (int64_t)P.bound};
  std::copy(out, out + 8, plan);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_NOMEM;
}

int lsspa_debug_cv_path_groups_plan(const int32_t* labels, int32_t p, int32_t g, int32_t K, int32_t L, int32_t block,
                                    int64_t* plan) try {
  GroupLayout G;
  if (!plan || g > GROUPS_MAX_G || p > GROUPS_MAX_P || K < 2 || K > CV_MAX_FOLDS || L < 1 || L > CV_PATH_MAX_REGS ||
      block < 0 || groups_layout(labels, p, g, G))
    return LSSPA_ERR_ARG;
  const CvPathPlan P = cv_path_groups_plan(G, K, L, block);
  const int64_t out[12] = {G.gl, G.gh, G.ql, G.nb, (int64_t)P.cut.units, (int64_t)P.cut.per,
                           (int64_t)P.cut.launch_steps(), P.block, P.blocks, P.reps, (int64_t)P.launches,
                           (int64_t)P.bound};
  std::copy(out, out + 12, plan);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_ARG;
}

}  // extern "C"

// ---- exact attribution of many responses at once (k_multi.hip) ------------------------------------------------------
// One reduction of Z = [X | Y] per side gives the shared G, H and every response's g_r, h_r, ||y_r||^2; the enumeration
// then runs blocks of responses, a block's chunks of MULTI_RB as the second grid dimension, into a partial table
// [chunks][MULTI_RB][units][p + 1] that launch_subsets_reduce sums in fixed order.  How often a unit's row is added to
// (the steps per launch) depends on p alone, so a response's bits do not depend on the block it runs in.
// lsspa_multi_groups_shapley (k_multi_groups.hip) is the same over groups of columns: the players are the g groups of a
// layout (groups_layout), the table [chunks][MULTI_RB][units][g + 1], the block loop multi_enumerate for both.
namespace {

// (high subset, chunk) passes one enumeration launch takes at most, over all units and chunks.  A pass carries MULTI_RB
// responses and costs 2.7 passes of k_subsets.hip (p = 28: 14.7 ms per 2^18 against 21.8 ms per 2^20; DESIGN.md, "Many
// responses at once"), whose launches take SUBSETS_PER_LAUNCH = 2^20 of them in ~35 ms at p = 32: a quarter of that
// keeps a launch inside the same bound (about 24 ms at p = 32).
constexpr uint64_t MULTI_PASSES_PER_LAUNCH = SUBSETS_PER_LAUNCH / 4;
constexpr size_t MULTI_TABLE_BYTES = 256ull << 20;     // the partial table of a block of responses stays inside this
constexpr int64_t MULTI_MAX_COLS = 32767;              // p + m
constexpr int64_t MULTI_MAX_CHUNKS = 8191;             // chunks * MULTI_RB is launch_subsets_reduce's replicate count

// m of a load against p (the loads of lsspa_multi_* and lsspa_multi_lift_*, after their own limit on p)
int multi_cols_limit(lsspa_ctx* ctx, const char* name, int64_t p, int64_t m) {
  if (m < 1 || p + m > MULTI_MAX_COLS) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s takes m >= 1 responses with p + m <= %lld (p = %lld, m = %lld given)", name,
             (long long)MULTI_MAX_COLS, (long long)p, (long long)m);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  return LSSPA_OK;
}

int multi_limits(lsspa_ctx* ctx, const char* name, int64_t p, int64_t m) {
  if (p < 1 || p > GROUPS_MAX_P) {       // (p > MULTI_MAX_P: for lsspa_multi_groups_shapley only, multi_need_ungrouped)
    char msg[200];
    snprintf(msg, sizeof msg, "%s takes 1 <= p <= %d columns, of which the ungrouped enumeration takes p <= %d "
             "(%lld given)", name, GROUPS_MAX_P, MULTI_MAX_P, (long long)p);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  return multi_cols_limit(ctx, name, p, m);
}

int multi_need_loaded(lsspa_ctx* ctx) {
  if (!ctx->multi.loaded)
    return ctx->fail(LSSPA_ERR_STATE, "no responses loaded (lsspa_multi_load or lsspa_multi_set_reduced comes first)");
  return LSSPA_OK;
}

// the enumeration over features takes p <= MULTI_MAX_P of the p <= GROUPS_MAX_P columns a load accepts
int multi_need_ungrouped(lsspa_ctx* ctx, const char* name) {
  if (ctx->multi.rf.p > MULTI_MAX_P) {
    char msg[240];
    snprintf(msg, sizeof msg, "%s enumerates all 2^p feature subsets and takes at most p = %d features (%d loaded); "
             "lsspa_multi_groups_shapley attributes to groups of up to %d columns", name, MULTI_MAX_P, ctx->multi.rf.p,
             GROUPS_MAX_P);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  return LSSPA_OK;
}

// responses enumerated together: as many as MULTI_TABLE_BYTES hold, whole chunks, at least one chunk.  n players
// (features, or groups of columns), n_high high subsets
int64_t multi_block_max(int n, uint64_t n_high) {
  const uint64_t units = exact_units(n_high);
  const int64_t fit = (int64_t)(MULTI_TABLE_BYTES / (units * (uint64_t)(n + 1) * sizeof(double)));
  const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>(fit / MULTI_RB, MULTI_MAX_CHUNKS));
  return chunks * MULTI_RB;
}

// the reduced form (host arrays: G, H [p][p], g, h [m][p], yy [m]) into the context
int multi_store(lsspa_ctx* ctx, int p, int m, const double* G, const double* g, const double* H, const double* h,
                const double* yy) {
  MultiWork& W = ctx->multi;
  W.loaded = false;
  TRY(reduced_check_yy(ctx, m, yy, "column %d of Y_test is identically zero (or NaN)"));
  TRY(reduced_store(ctx, W.rf, p, m, G, g, H, h, yy, W.rf.g, W.rf.h));
  std::vector<double> inv((size_t)m);
  for (int r = 0; r < m; ++r) inv[r] = 1.0 / yy[r];
  TRY(dev_alloc(ctx, W.inv_yy, (size_t)m));
  HIPCHK(hipMemcpy(W.inv_yy.ptr, inv.data(), sizeof(double) * m, hipMemcpyHostToDevice));
  W.loaded = true;
  return LSSPA_OK;
}

// The kernels' view of the loaded responses first .. first + count - 1: weights on the device, a cleared info word
int multi_args(lsspa_ctx* ctx, MultiWork& W, int64_t first, int64_t count, MultiArgs& a) {
  const int p = W.rf.p;
  constexpr int WR = EXACT_MAX_PLAYERS + 1;
  double w[EXACT_W_ROWS * WR];
  exact_weight_table(p, w);
  TRY(dev_alloc(ctx, W.w, EXACT_W_ROWS * WR));
  TRY(dev_alloc(ctx, W.info, 8));
  HIPCHK(hipStreamSynchronize(ctx->stream));     // a previous call may still read W.w; the copy is from a host frame
  HIPCHK(hipMemcpy(W.w.ptr, w, sizeof w, hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(W.info.ptr, 0, 8 * sizeof(int32_t), ctx->stream));
  a = MultiArgs{};
  a.G = W.rf.G.ptr;
  a.H = W.rf.H.ptr;
  a.ldg = a.ldh = p;
  a.g = W.rf.g.ptr + (size_t)first * p;
  a.h = W.rf.h.ptr + (size_t)first * p;
  a.inv_yy = W.inv_yy.ptr + first;
  a.w = W.w.ptr;
  a.p = p;
  a.q = subsets_low_features(p);
  a.count = (int)count;
  a.piv_tol = exact_piv_tol(p);
  a.info = W.info.ptr;
  return LSSPA_OK;
}

// first, count, block of an enumeration call against the responses loaded
int multi_range(lsspa_ctx* ctx, const MultiWork& W, const char* name, int64_t first, int64_t count, int64_t block) {
  const int m = W.rf.m;
  if (first < 0 || count < 1 || first > m || count > m - first || block < 0) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: responses first = %lld, count = %lld must lie inside the %d loaded, "
             "count >= 1, block >= 0", name, (long long)first, (long long)count, m);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  return LSSPA_OK;
}

// The enumeration of `count` responses, shared by the calls over features and over groups: n players, n_high high subsets
// in exact_units(n_high) units, blocks of responses as MULTI_TABLE_BYTES hold (or `block`), at most `passes` (high subset,
// chunk) passes a launch.  launch(r0, cnt, part, units, s0, s1): steps s0 .. s1 - 1 of every unit for the cnt responses
// from r0 (among those of the call) into part; store(r, out): the n + 1 column sums of response r's table.  The steps a
// launch takes depend on n_high and passes alone, so a response's bits do not depend on the block it runs in.  Leaves the
// call's timing in W and the info word in info (may be NULL).  W: the responses' owner (ctx->multi, or the permutation
// test's own).
template <typename Launch, typename Store>
int multi_enumerate(lsspa_ctx* ctx, MultiWork& W, int n, uint64_t n_high, uint64_t passes, int64_t count, int64_t block,
                    Launch&& launch, Store&& store, int32_t* info) {
  const int64_t bmax = multi_block_max(n, n_high);
  const int64_t blk = std::min<int64_t>(block == 0 ? bmax : std::min(block, bmax), count);
  const uint64_t units = exact_units(n_high), per = n_high / units;
  // steps per launch by the players alone; the chunks of a launch make up the rest of its bound
  const uint64_t steps = std::min(per, std::max<uint64_t>(1, passes / units));
  const int64_t chunks_per_launch = (int64_t)std::max<uint64_t>(1, passes / (units * steps));
  const size_t c = (size_t)n + 1;
  const int64_t max_chunks = (blk + MULTI_RB - 1) / MULTI_RB;
  TRY(dev_alloc(ctx, W.part, (size_t)max_chunks * MULTI_RB * units * c));
  TRY(dev_alloc(ctx, W.out, (size_t)max_chunks * MULTI_RB * c));
  std::vector<double> out((size_t)max_chunks * MULTI_RB * c);
  std::vector<hipEvent_t> ev;
  Events guard{ev};
  W.enum_ms = W.max_launch_ms = 0.0;
  W.launches = 0;
  for (int64_t b0 = 0; b0 < count; b0 += blk) {
    const int64_t nb = std::min(blk, count - b0);
    const int64_t chunks = (nb + MULTI_RB - 1) / MULTI_RB;
    HIPCHK(hipMemsetAsync(W.part.ptr, 0, sizeof(double) * (size_t)chunks * MULTI_RB * units * c, ctx->stream));
    const size_t e0 = ev.size();
    ev.push_back(nullptr);
    HIPCHK(hipEventCreate(&ev.back()));
    HIPCHK(hipEventRecord(ev.back(), ctx->stream));
    for (int64_t c0 = 0; c0 < chunks; c0 += chunks_per_launch) {
      const int64_t r0 = b0 + c0 * MULTI_RB;                 // the launch's first response, among those of the call
      const int64_t cnt = std::min<int64_t>(chunks_per_launch * MULTI_RB, b0 + nb - r0);
      double* part = W.part.ptr + (size_t)c0 * MULTI_RB * units * c;
      for (uint64_t s0 = 0; s0 < per; s0 += steps) {
        HIPCHK(launch(r0, cnt, part, units, s0, std::min(per, s0 + steps)));
        ev.push_back(nullptr);
        HIPCHK(hipEventCreate(&ev.back()));
        HIPCHK(hipEventRecord(ev.back(), ctx->stream));
      }
    }
    HIPCHK(launch_subsets_reduce(W.part.ptr, (int64_t)units, (int)c, W.out.ptr, ctx->stream, (int)(chunks * MULTI_RB)));
    HIPCHK(hipMemcpyAsync(out.data(), W.out.ptr, sizeof(double) * (size_t)nb * c, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int64_t r = 0; r < nb; ++r) store(b0 + r, out.data() + (size_t)r * c);
    for (size_t k = e0; k + 1 < ev.size(); ++k) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
      W.enum_ms += ms;
      W.max_launch_ms = std::max(W.max_launch_ms, (double)ms);
      ++W.launches;
    }
    for (hipEvent_t& e : ev) {
      (void)hipEventDestroy(e);
      e = nullptr;
    }
    ev.clear();
  }
  int32_t bits = 0;
  HIPCHK(hipMemcpy(&bits, W.info.ptr, sizeof bits, hipMemcpyDeviceToHost));
  if (info) *info = bits;
  return LSSPA_OK;
}

// The grouped kernels' view of the loaded responses first .. first + count - 1: the layout L of the labels and its table
// on the device, the weights of g players, a cleared info word
int multi_group_args(lsspa_ctx* ctx, MultiWork& W, const int32_t* labels, int32_t g, int64_t first, int64_t count,
                     MultiGroupArgs& a, GroupLayout& L) {
  const int p = W.rf.p;
  char msg[200];
  if (g > GROUPS_MAX_G) {
    snprintf(msg, sizeof msg, "exact attribution over groups takes at most g = %d groups (%d given)", GROUPS_MAX_G,
             (int)g);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  if (const char* why = groups_layout(labels, p, g, L)) {
    snprintf(msg, sizeof msg, "group labels: %s", why);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  constexpr int WR = EXACT_MAX_PLAYERS + 1;
  double w[EXACT_W_ROWS * WR];
  exact_weight_table(L.ng, w);
  TRY(dev_alloc(ctx, W.w, EXACT_W_ROWS * WR));
  TRY(dev_alloc(ctx, W.tab, GROUPS_TAB_LEN));
  TRY(dev_alloc(ctx, W.info, 8));
  HIPCHK(hipStreamSynchronize(ctx->stream));     // a previous call may still read W.w / W.tab; the copies are from host frames
  HIPCHK(hipMemcpy(W.w.ptr, w, sizeof w, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(W.tab.ptr, L.tab, GROUPS_TAB_LEN * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(W.info.ptr, 0, 8 * sizeof(int32_t), ctx->stream));
  a = MultiGroupArgs{};
  a.G = W.rf.G.ptr;
  a.H = W.rf.H.ptr;
  a.ldg = a.ldh = p;
  a.g = W.rf.g.ptr + (size_t)first * p;
  a.h = W.rf.h.ptr + (size_t)first * p;
  a.inv_yy = W.inv_yy.ptr + first;
  a.w = W.w.ptr;
  a.tab = W.tab.ptr;
  a.p = p; a.ng = L.ng; a.nb = L.nb;
  a.gl = L.gl; a.gh = L.gh; a.ql = L.ql;
  a.count = (int)count;
  a.piv_tol = exact_piv_tol(p);
  a.info = W.info.ptr;
  return LSSPA_OK;
}

// frees what a load borrows from the device on every way out
struct MultiScratch {
  DevBuf<char> zx, yl;
  DevBuf<double> C;
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~MultiScratch() {
    dev_free(zx);
    dev_free(yl);
    dev_free(C);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// the array arguments of a load from the rows (lsspa_multi_load, lsspa_multi_lift_load)
bool multi_sides_ok(const void* X_train, int64_t ld_train, const void* Y_train, int64_t ldy_train, int64_t N,
                    const void* X_test, int64_t ld_test, const void* Y_test, int64_t ldy_test, int64_t M, int32_t p,
                    int32_t m, double reg, int32_t dtype, int32_t location) {
  return !(!X_train || !Y_train || !X_test || !Y_test || N < 1 || M < 1 || ld_train < p || ld_test < p || ldy_train < m ||
           ldy_test < m || !(reg >= 0.0) || !std::isfinite(reg) || (dtype != LSSPA_F64 && dtype != LSSPA_F32) ||
           (location != LSSPA_HOST && location != LSSPA_DEVICE));
}

// One Gram pass per side over Z = [X | Y] -> the reduced form on the host: G = X^T X / N + reg I and H = X_te^T X_te
// [p][p], g = X^T Y / N and h = X_te^T Y_te [m][p], yy [m] = the test responses' squared norms; gram_ms: the two passes'
// kernel time.  The arguments have been checked (multi_sides_ok and the caller's limits).
int multi_reduce_sides(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* Y_train, int64_t ldy_train,
                       int64_t N, const void* X_test, int64_t ld_test, const void* Y_test, int64_t ldy_test, int64_t M,
                       int32_t p, int32_t m, double reg, int32_t dtype, int32_t location, std::vector<double>& G,
                       std::vector<double>& g, std::vector<double>& H, std::vector<double>& h, std::vector<double>& yy,
                       double& gram_ms) {
  const size_t es = dtype == LSSPA_F32 ? 4 : 8;
  const int cols = p + m - 1;                      // launch_gram's "features": Z = [X | Y] has cols + 1 columns
  const size_t P1pad = (size_t)round_up(p + m, 128);
  const hipMemcpyKind kind = location == LSSPA_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  MultiScratch S;
  TRY(dev_alloc(ctx, S.C, P1pad * P1pad));
  for (hipEvent_t& e : S.ev) HIPCHK(hipEventCreate(&e));
  const void* X[2] = {X_train, X_test};
  const void* Y[2] = {Y_train, Y_test};
  const int64_t n[2] = {N, M}, ld[2] = {ld_train, ld_test}, ldy[2] = {ldy_train, ldy_test};
  std::vector<double> rows[2], cross[2];
  yy.assign((size_t)m, 0.0);
  gram_ms = 0.0;
  for (int s = 0; s < 2; ++s) {
    // [X | Y[:, :m-1]] as launch_gram's X and Y's last column as its y
    TRY(dev_alloc(ctx, S.zx, (size_t)n[s] * cols * es));
    TRY(dev_alloc(ctx, S.yl, (size_t)n[s] * es));
    HIPCHK(hipMemcpy2DAsync(S.zx.ptr, (size_t)cols * es, X[s], (size_t)ld[s] * es, (size_t)p * es, (size_t)n[s], kind,
                            ctx->stream));
    if (m > 1)
      HIPCHK(hipMemcpy2DAsync(S.zx.ptr + (size_t)p * es, (size_t)cols * es, Y[s], (size_t)ldy[s] * es,
                              (size_t)(m - 1) * es, (size_t)n[s], kind, ctx->stream));
    HIPCHK(hipMemcpy2DAsync(S.yl.ptr, es, (const char*)Y[s] + (size_t)(m - 1) * es, (size_t)ldy[s] * es, es,
                            (size_t)n[s], kind, ctx->stream));
    HIPCHK(hipMemsetAsync(S.C.ptr, 0, sizeof(double) * P1pad * P1pad, ctx->stream));
    HIPCHK(hipEventRecord(S.ev[0], ctx->stream));
    TRY(gram_side(ctx, S.zx.ptr, S.yl.ptr, n[s], cols, cols, dtype == LSSPA_F32, S.C.ptr));
    HIPCHK(hipEventRecord(S.ev[1], ctx->stream));
    // launch_gram leaves the lower part (row >= column) of a diagonal tile: G, H from rows < p, the responses' sums from
    // the first p columns of rows p .. p + m - 1
    rows[s].resize((size_t)p * P1pad);
    cross[s].resize((size_t)m * p);
    HIPCHK(hipMemcpyAsync(rows[s].data(), S.C.ptr, sizeof(double) * p * P1pad, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpy2DAsync(cross[s].data(), sizeof(double) * p, S.C.ptr + (size_t)p * P1pad, sizeof(double) * P1pad,
                            sizeof(double) * p, (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    if (s == 1)
      HIPCHK(hipMemcpy2DAsync(yy.data(), sizeof(double), S.C.ptr + (size_t)p * P1pad + p, sizeof(double) * (P1pad + 1),
                              sizeof(double), (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
    gram_ms += ms;
  }
  const double scale = 1.0 / (double)N;
  G.assign((size_t)p * p, 0.0);
  H.assign((size_t)p * p, 0.0);
  g.assign((size_t)m * p, 0.0);
  h.assign((size_t)m * p, 0.0);
  for (int a = 0; a < p; ++a) {
    for (int b = 0; b < p; ++b) {
      const size_t lo = a >= b ? a * P1pad + b : b * P1pad + a;
      G[(size_t)a * p + b] = rows[0][lo] * scale + (a == b ? reg : 0.0);
      H[(size_t)a * p + b] = rows[1][lo];
    }
    for (int r = 0; r < m; ++r) {
      g[(size_t)r * p + a] = cross[0][(size_t)r * p + a] * scale;
      h[(size_t)r * p + a] = cross[1][(size_t)r * p + a];
    }
  }
  return LSSPA_OK;
}

// lsspa_multi_shapley on the responses of W (checked: loaded, p <= MULTI_MAX_P, phi, the range)
int multi_shapley_on(lsspa_ctx* ctx, MultiWork& W, int64_t first, int64_t count, int64_t block, double* phi,
                     int32_t* info) {
  const int p = W.rf.p;
  HIPCHK(hipSetDevice(ctx->device));
  const int q = subsets_low_features(p);
  const uint64_t n_high = 1ull << (p - q);
  MultiArgs a;
  TRY(multi_args(ctx, W, first, count, a));
  a.per = n_high / exact_units(n_high);
  auto launch = [&](int64_t r0, int64_t cnt, double* part, uint64_t units, uint64_t s0, uint64_t s1) {
    MultiArgs l = a;
    l.g = a.g + (size_t)r0 * p;
    l.h = a.h + (size_t)r0 * p;
    l.inv_yy = a.inv_yy + r0;
    l.count = (int)cnt;
    l.part = part;
    return launch_multi_enum(l, units, s0, s1, ctx->stream);
  };
  auto store = [&](int64_t r, const double* out) {
    for (int j = 0; j < p; ++j) phi[(size_t)r * p + j] = out[j] - out[p];
  };
  return multi_enumerate(ctx, W, p, n_high, MULTI_PASSES_PER_LAUNCH, count, block, launch, store, info);
}

// lsspa_multi_groups_shapley on the responses of W (checked: loaded, labels, phi, the range)
int multi_groups_shapley_on(lsspa_ctx* ctx, MultiWork& W, const int32_t* labels, int32_t g, int64_t first, int64_t count,
                            int64_t block, double* phi, int32_t* info) {
  const int p = W.rf.p;
  HIPCHK(hipSetDevice(ctx->device));
  MultiGroupArgs a;
  GroupLayout L;
  TRY(multi_group_args(ctx, W, labels, g, first, count, a, L));
  const int ng = L.ng;
  const uint64_t n_high = 1ull << L.gh;
  a.per = n_high / exact_units(n_high);
  // passes per launch: groups_enumerate's bound by the rows of a subset's matrix, a quarter of it as a pass carries
  // MULTI_RB responses (MULTI_PASSES_PER_LAUNCH); by the layout alone, so a response's bits do not depend on the block
  const uint64_t rows = (uint64_t)(L.nb + L.ql + 1) + (uint64_t)(L.p - L.nb - L.ql + 1) / 2;
  const uint64_t passes = std::max<uint64_t>(1, GROUPS_WORK_PER_LAUNCH / (rows * rows) / 4);
  auto launch = [&](int64_t r0, int64_t cnt, double* part, uint64_t units, uint64_t s0, uint64_t s1) {
    MultiGroupArgs l = a;
    l.g = a.g + (size_t)r0 * p;
    l.h = a.h + (size_t)r0 * p;
    l.inv_yy = a.inv_yy + r0;
    l.count = (int)cnt;
    l.part = part;
    return launch_multi_groups_enum(l, units, s0, s1, ctx->stream);
  };
  auto store = [&](int64_t r, const double* out) {
    for (int k = 0; k < ng; ++k) phi[(size_t)r * ng + L.gid[k]] = out[k] - out[ng];
  };
  return multi_enumerate(ctx, W, ng, n_high, passes, count, block, launch, store, info);
}

}  // namespace

extern "C" {

int lsspa_multi_load(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* Y_train, int64_t ldy_train,
                     int64_t N, const void* X_test, int64_t ld_test, const void* Y_test, int64_t ldy_test, int64_t M,
                     int32_t p, int32_t m, double reg, int32_t dtype, int32_t location) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(multi_limits(ctx, "lsspa_multi_load", p, m));
  if (!multi_sides_ok(X_train, ld_train, Y_train, ldy_train, N, X_test, ld_test, Y_test, ldy_test, M, p, m, reg, dtype,
                      location))
    return ctx->fail(LSSPA_ERR_ARG, "lsspa_multi_load: NULL array, N or M < 1, ld < p, ldy < m, reg not finite and >= 0, "
                                    "or bad dtype / location");
  HIPCHK(hipSetDevice(ctx->device));
  MultiWork& W = ctx->multi;
  W.loaded = false;
  std::vector<double> G, g, H, h, yy;
  TRY(multi_reduce_sides(ctx, X_train, ld_train, Y_train, ldy_train, N, X_test, ld_test, Y_test, ldy_test, M, p, m, reg,
                         dtype, location, G, g, H, h, yy, W.gram_ms));
  return multi_store(ctx, p, m, G.data(), g.data(), H.data(), h.data(), yy.data());
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_multi_set_reduced(lsspa_ctx* ctx, int32_t p, int32_t m, const double* G, const double* g, const double* H,
                            const double* h, const double* yy) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(multi_limits(ctx, "lsspa_multi_set_reduced", p, m));
  if (!G || !g || !H || !h || !yy) return ctx->fail(LSSPA_ERR_ARG, "lsspa_multi_set_reduced: NULL array");
  HIPCHK(hipSetDevice(ctx->device));
  ctx->multi.gram_ms = 0.0;
  return multi_store(ctx, p, m, G, g, H, h, yy);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_multi_shapley(lsspa_ctx* ctx, int64_t first, int64_t count, int64_t block, double* phi, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(multi_need_loaded(ctx));
  TRY(multi_need_ungrouped(ctx, "lsspa_multi_shapley"));
  MultiWork& W = ctx->multi;
  if (!phi) return ctx->fail(LSSPA_ERR_ARG, "lsspa_multi_shapley: phi is NULL");
  TRY(multi_range(ctx, W, "lsspa_multi_shapley", first, count, block));
  return multi_shapley_on(ctx, W, first, count, block, phi, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_multi_groups_shapley(lsspa_ctx* ctx, const int32_t* labels, int32_t g, int64_t first, int64_t count,
                               int64_t block, double* phi, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(multi_need_loaded(ctx));
  MultiWork& W = ctx->multi;
  if (!phi || !labels) return ctx->fail(LSSPA_ERR_ARG, "lsspa_multi_groups_shapley: labels / phi is NULL");
  TRY(multi_range(ctx, W, "lsspa_multi_groups_shapley", first, count, block));
  return multi_groups_shapley_on(ctx, W, labels, g, first, count, block, phi, info);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_multi_get_gram(lsspa_ctx* ctx, double* G, double* g, double* H, double* h, double* yy) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(multi_need_loaded(ctx));
  reduced_get(ctx->multi.rf, G, g, H, h, yy);
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_multi_timing(const lsspa_ctx* ctx, double* gram_ms, double* enum_ms, double* max_launch_ms,
                       int64_t* launches) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (gram_ms) *gram_ms = ctx->multi.gram_ms;
  if (enum_ms) *enum_ms = ctx->multi.enum_ms;
  if (max_launch_ms) *max_launch_ms = ctx->multi.max_launch_ms;
  if (launches) *launches = ctx->multi.launches;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(const_cast<lsspa_ctx*>(ctx));
}

int lsspa_multi_free(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->multi.release();
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_multi_values(lsspa_ctx* ctx, const uint64_t* masks, int64_t n, double* v) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(multi_need_loaded(ctx));
  TRY(multi_need_ungrouped(ctx, "lsspa_debug_multi_values"));
  MultiWork& W = ctx->multi;
  if (n < 0 || (n > 0 && (!masks || !v))) return ctx->fail(LSSPA_ERR_ARG, "masks / v NULL or n < 0");
  const uint64_t full = (1ull << W.rf.p) - 1ull;     // p <= 32 here
  for (int64_t i = 0; i < n; ++i)
    if (masks[i] & ~full) return ctx->fail(LSSPA_ERR_ARG, "a mask names a feature beyond p");
  if (n == 0) return LSSPA_OK;
  HIPCHK(hipSetDevice(ctx->device));
  const int m = W.rf.m;
  MultiArgs a;
  TRY(multi_args(ctx, W, 0, m, a));
  TRY(dev_alloc(ctx, W.masks, (size_t)n));
  TRY(dev_alloc(ctx, W.vals, (size_t)n * m));
  HIPCHK(hipMemcpy(W.masks.ptr, masks, sizeof(uint64_t) * n, hipMemcpyHostToDevice));
  HIPCHK(launch_multi_debug(a, W.masks.ptr, n, W.vals.ptr, m, 0, ctx->stream));
  HIPCHK(hipMemcpyAsync(v, W.vals.ptr, sizeof(double) * (size_t)n * m, hipMemcpyDeviceToHost, ctx->stream));
  int32_t bits = 0;
  HIPCHK(hipMemcpyAsync(&bits, W.info.ptr, sizeof bits, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (bits & LSSPA_INFO_NOT_PD) return ctx->fail(LSSPA_ERR_STATE, "a subset's Gram matrix is not positive definite");
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_multi_group_values(lsspa_ctx* ctx, const int32_t* labels, int32_t g, const uint64_t* masks, int64_t n,
                                   double* u) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(multi_need_loaded(ctx));
  MultiWork& W = ctx->multi;
  if (!labels || n < 0 || (n > 0 && (!masks || !u))) return ctx->fail(LSSPA_ERR_ARG, "labels / masks / u NULL or n < 0");
  HIPCHK(hipSetDevice(ctx->device));
  const int m = W.rf.m;
  MultiGroupArgs a;
  GroupLayout L;
  TRY(multi_group_args(ctx, W, labels, g, 0, m, a, L));
  const uint64_t full = (1ull << L.ng) - 1ull;     // g <= 32
  for (int64_t i = 0; i < n; ++i)
    if (masks[i] & ~full) return ctx->fail(LSSPA_ERR_ARG, "a mask names a group beyond g");
  if (n == 0) return LSSPA_OK;
  const std::vector<uint64_t> lay = layout_masks(L, masks, n);
  TRY(dev_alloc(ctx, W.masks, (size_t)n));
  TRY(dev_alloc(ctx, W.vals, (size_t)n * m));
  HIPCHK(hipMemcpy(W.masks.ptr, lay.data(), sizeof(uint64_t) * n, hipMemcpyHostToDevice));
  HIPCHK(launch_multi_groups_debug(a, W.masks.ptr, n, W.vals.ptr, m, 0, ctx->stream));
  HIPCHK(hipMemcpyAsync(u, W.vals.ptr, sizeof(double) * (size_t)n * m, hipMemcpyDeviceToHost, ctx->stream));
  int32_t bits = 0;
  HIPCHK(hipMemcpyAsync(&bits, W.info.ptr, sizeof bits, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (bits & LSSPA_INFO_NOT_PD)
    return ctx->fail(LSSPA_ERR_STATE, "a group subset's Gram matrix is not positive definite");
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

}  // extern "C"

// ---- what the three sampled families share: player map, orderings, running statistics, launch timing, problem store ----
namespace {

// lsspa_*_lift_set_players on the family's map: the refusals, quiesce() (the family's wait for the stream, and what it
// resets with it), the upload.  The map changes what a sample is, so the caller starts its statistics or orderings over.
template <typename Quiesce>
int lift_players_set(lsspa_ctx* ctx, LiftPlayers& P, const char* entry, int p, const int32_t* labels, int g,
                     Quiesce&& quiesce) {
  char msg[120];
  snprintf(msg, sizeof msg, "%s: labels is NULL (clear the map with labels = NULL, g = 0)", entry);
  return player_map_set(ctx, msg, labels, p, g, quiesce, P.map, P.pl_off, P.pl_cols, P.ng);
}

int lift_check_orderings(lsspa_ctx* ctx, const char* entry, const char* count_name, const int32_t* perms, int64_t count,
                         int p, int g, int d, int limit_rows) {
  char msg[240];
  if (lift_orderings_why(entry, count_name, perms, count, p, g, d, limit_rows, ctx->perm_mark, msg, sizeof msg))
    return ctx->fail(LSSPA_ERR_ARG, msg);
  return LSSPA_OK;
}

int lift_stats_alloc(lsspa_ctx* ctx, LiftStats& S, size_t entries) {
  TRY(dev_alloc(ctx, S.mean, entries));
  return dev_alloc(ctx, S.M2, entries);
}
// n = 0, (mean, M2) cleared; the caller has waited for the stream
int lift_stats_clear(lsspa_ctx* ctx, LiftStats& S, size_t entries) {
  HIPCHK(hipMemset(S.mean.ptr, 0, sizeof(double) * entries));
  HIPCHK(hipMemset(S.M2.ptr, 0, sizeof(double) * entries));
  S.n = 0;
  return LSSPA_OK;
}
// lsspa_*_lift_reset: the wait, the clear, and the family's info words
int lift_stats_reset(lsspa_ctx* ctx, LiftStats& S, size_t entries, DevBuf<int32_t>& info, size_t n_info) {
  HIPCHK(hipStreamSynchronize(ctx->stream));
  TRY(lift_stats_clear(ctx, S, entries));
  HIPCHK(hipMemset(info.ptr, 0, sizeof(int32_t) * n_info));
  return LSSPA_OK;
}
// ns samples [ns][entries] into the running state
int lift_stats_fold(lsspa_ctx* ctx, LiftStats& S, const double* samples, int64_t entries, int64_t ns) {
  HIPCHK(launch_multi_lift_stats(samples, entries, (int)ns, S.n, S.mean.ptr, S.M2.ptr, ctx->stream));
  S.n += ns;
  return LSSPA_OK;
}
// lsspa_*_lift_get
int lift_stats_get(lsspa_ctx* ctx, const LiftStats& S, size_t entries, int64_t* n, double* mean, double* m2) {
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (n) *n = S.n;
  if (mean) HIPCHK(hipMemcpy(mean, S.mean.ptr, sizeof(double) * entries, hipMemcpyDeviceToHost));
  if (m2) HIPCHK(hipMemcpy(m2, S.M2.ptr, sizeof(double) * entries, hipMemcpyDeviceToHost));
  return LSSPA_OK;
}

// A batch launch's three events: the lift kernels between mark 0 and mark 1, what folds their output between 1 and 2.
// finish() waits for the stream (the next launch reuses the buffers) and gives the two intervals.
struct LiftLaunchTimer {
  std::vector<hipEvent_t> ev = std::vector<hipEvent_t>(3, nullptr);
  Events guard{ev};
  int create(lsspa_ctx* ctx) {
    for (hipEvent_t& e : ev) HIPCHK(hipEventCreate(&e));
    return LSSPA_OK;
  }
  int mark(lsspa_ctx* ctx, int k) {
    HIPCHK(hipEventRecord(ev[(size_t)k], ctx->stream));
    return LSSPA_OK;
  }
  int finish(lsspa_ctx* ctx, double& lift_ms, double& fold_ms) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    lift_ms = ms;
    HIPCHK(hipEventElapsedTime(&ms, ev[1], ev[2]));
    fold_ms = ms;
    return LSSPA_OK;
  }
};

// room for `count` problems; inv_yy takes `small` entries and aug twice as many
int lift_problems_alloc(lsspa_ctx* ctx, LiftProblems& Q, size_t count, size_t small) {
  TRY(dev_alloc(ctx, Q.G, count * LiftProblems::LL));
  TRY(dev_alloc(ctx, Q.H, count * LiftProblems::LL));
  TRY(dev_alloc(ctx, Q.g, count * LiftProblems::LD));
  TRY(dev_alloc(ctx, Q.h, count * LiftProblems::LD));
  TRY(dev_alloc(ctx, Q.inv_yy, small));
  return dev_alloc(ctx, Q.aug, 2 * small);
}
// the columns behind p of a problem's rows are read (the register-resident gather fetches pairs), never used: zero
int lift_problems_zero(lsspa_ctx* ctx, LiftProblems& Q, size_t count, hipStream_t st) {
  HIPCHK(hipMemsetAsync(Q.G.ptr, 0, sizeof(double) * count * LiftProblems::LL, st));
  HIPCHK(hipMemsetAsync(Q.H.ptr, 0, sizeof(double) * count * LiftProblems::LL, st));
  HIPCHK(hipMemsetAsync(Q.g.ptr, 0, sizeof(double) * count * LiftProblems::LD, st));
  HIPCHK(hipMemsetAsync(Q.h.ptr, 0, sizeof(double) * count * LiftProblems::LD, st));
  return LSSPA_OK;
}
// problems first .. first + n - 1 dense to the host, enqueued on st: G, H [n][p][p], g, h [n][p], inv_yy [n]; any may be NULL
int lift_problems_copy_out(lsspa_ctx* ctx, const LiftProblems& Q, int64_t first, int64_t n, int p, double* G, double* H,
                           double* g, double* h, double* inv_yy, hipStream_t st) {
  constexpr size_t LD = LiftProblems::LD, LL = LiftProblems::LL, row = sizeof(double) * LD;
  const size_t w = sizeof(double) * p, pp = (size_t)p * p;
  for (int64_t f = 0; f < n; ++f) {
    if (G) HIPCHK(hipMemcpy2DAsync(G + f * pp, w, Q.G.ptr + (first + f) * LL, row, w, (size_t)p, hipMemcpyDeviceToHost, st));
    if (H) HIPCHK(hipMemcpy2DAsync(H + f * pp, w, Q.H.ptr + (first + f) * LL, row, w, (size_t)p, hipMemcpyDeviceToHost, st));
  }
  if (g) HIPCHK(hipMemcpy2DAsync(g, w, Q.g.ptr + first * LD, row, w, (size_t)n, hipMemcpyDeviceToHost, st));
  if (h) HIPCHK(hipMemcpy2DAsync(h, w, Q.h.ptr + first * LD, row, w, (size_t)n, hipMemcpyDeviceToHost, st));
  if (inv_yy) HIPCHK(hipMemcpyAsync(inv_yy, Q.inv_yy.ptr + first, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  return LSSPA_OK;
}
// What launch_small_folds / launch_small_problems take of an ordering launch over stored problems, whoever calls: the
// orderings' form (with a map both rows of a pair are explicit -- the baseline stays first) and the raw lifts ...
SmallArgs lift_small_args(int p, int nb, int per, int g, double* raw) {
  SmallArgs a{};
  a.ld_src = LiftProblems::LD;
  a.fwd_only = (!g && per == 2) ? 1 : 0;
  a.p = p;
  a.nb = nb;
  a.per_sample = per;
  a.lifts = raw;
  a.y_norm_sq = 1.0;
  a.piv_tol = exact_piv_tol(p);
  a.sum_tol = -1.0;
  return a;
}
// ... and problems first .. first + folds - 1 of the store
void lift_problems_args(const LiftProblems& Q, int64_t first, int folds, SmallArgs& a, SmallFolds& fo) {
  a.S[0] = Q.G.ptr + first * LiftProblems::LL;
  a.S[1] = Q.H.ptr + first * LiftProblems::LL;
  a.s[0] = Q.g.ptr + first * LiftProblems::LD;
  a.s[1] = Q.h.ptr + first * LiftProblems::LD;
  fo.mat = LiftProblems::LL;
  fo.vec = LiftProblems::LD;
  fo.aug = Q.aug.ptr + 2 * first;
  fo.inv_yy = Q.inv_yy.ptr + first;
  fo.folds = folds;
}

}  // namespace

// ---- sampled attribution of many responses on one design matrix (k_small_multi.hip) ----------------------------------
// The reduced form is lsspa_multi_load's (one Gram pass per side over Z = [X | Y]).  A batch of orderings runs as
// launches of whole samples, a launch's grid (orderings of its samples) x (chunks of MLIFT_RB responses); its lift vectors
// [samples][m][p] are folded into the running (n, mean, M2) [m][p] by a launch of their own and copied out if asked for.
// With a player map the orderings are orderings of the g groups, expanded on the host as they are staged (two rows a
// sample when antithetical), and the kernel folds each response's lifts to g group lifts itself: [samples][m][g].
namespace {

constexpr int64_t MLIFT_GRID_PER_LAUNCH = 1 << 16;            // workgroups a launch takes at most (one sample at least)
constexpr int64_t MLIFT_LIFT_DOUBLES = (256ll << 20) / 8;     // lift vectors of a launch: 256 MB at most (one sample at least)

int mlift_limits(lsspa_ctx* ctx, const char* name, int64_t p, int64_t m) {
  if (p < 1 || p > MLIFT_MAX_P) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s takes 1 <= p <= %d features (%lld given): both work matrices and %d augmented rows "
             "stay in a compute unit's LDS", name, MLIFT_MAX_P, (long long)p, MLIFT_RB);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  return multi_cols_limit(ctx, name, p, m);
}

int mlift_need_loaded(lsspa_ctx* ctx) {
  if (!ctx->mlift.loaded)
    return ctx->fail(LSSPA_ERR_STATE, "no responses loaded (lsspa_multi_lift_load or lsspa_multi_lift_set_reduced comes "
                                      "first)");
  return LSSPA_OK;
}

// max over the responses of ||L^-1 b_r||^2, A = L L^T [p][p], b [m][p]: what the diagonal of the augmented rows has to
// exceed (MultiLiftArgs::aug).  A pivot that is not positive is replaced by 1, as the kernels do (they flag it).
double mlift_rhs_bound(int p, int m, const double* A, const double* b) {
  std::vector<double> L(A, A + (size_t)p * p), z((size_t)p);
  for (int j = 0; j < p; ++j) {
    double d = L[(size_t)j * p + j];
    for (int k = 0; k < j; ++k) d -= L[(size_t)j * p + k] * L[(size_t)j * p + k];
    if (!(d > 0.0) || !std::isfinite(d)) d = 1.0;
    const double ljj = std::sqrt(d);
    L[(size_t)j * p + j] = ljj;
    for (int i = j + 1; i < p; ++i) {
      double v = L[(size_t)i * p + j];
      for (int k = 0; k < j; ++k) v -= L[(size_t)i * p + k] * L[(size_t)j * p + k];
      L[(size_t)i * p + j] = v / ljj;
    }
  }
  double worst = 0.0;
  for (int r = 0; r < m; ++r) {
    double nn = 0.0;
    for (int i = 0; i < p; ++i) {
      double v = b[(size_t)r * p + i];
      for (int k = 0; k < i; ++k) v -= L[(size_t)i * p + k] * z[k];
      z[i] = v / L[(size_t)i * p + i];
      nn += z[i] * z[i];
    }
    if (nn > worst) worst = nn;
  }
  return std::isfinite(worst) ? worst : 0.0;
}

// the reduced form (host arrays: G, H [p][p], g, h [m][p], yy [m]) into the context; statistics and info word cleared
int mlift_store(lsspa_ctx* ctx, int p, int m, const double* G, const double* g, const double* H, const double* h,
                const double* yy) {
  MultiLiftWork& W = ctx->mlift;
  W.loaded = false;
  W.pl.ng = 0;             // a player map belongs to the responses it was set on
  TRY(reduced_check_yy(ctx, m, yy, "column %d of Y_test is identically zero (or NaN)"));
  // the augmented rows' trailing corner  aug I - Z Z^T  (Z: the z rows of a chunk) stays positive definite when aug
  // exceeds the sum of the chunk's ||z_r||^2: twice MLIFT_RB times the largest, plus one
  W.aug[0] = 1.0 + 2.0 * MLIFT_RB * mlift_rhs_bound(p, m, G, g);
  W.aug[1] = 1.0 + 2.0 * MLIFT_RB * mlift_rhs_bound(p, m, H, h);
  TRY(reduced_store(ctx, W.rf, p, m, G, g, H, h, yy, W.rf.g, W.rf.h));
  const size_t mp = (size_t)m * p;
  TRY(dev_alloc(ctx, W.yy, (size_t)m));
  TRY(lift_stats_alloc(ctx, W.st, mp));
  TRY(dev_alloc(ctx, W.info, 8));
  HIPCHK(hipMemcpy(W.yy.ptr, yy, sizeof(double) * m, hipMemcpyHostToDevice));
  TRY(lift_stats_clear(ctx, W.st, mp));
  HIPCHK(hipMemset(W.info.ptr, 0, 8 * sizeof(int32_t)));
  W.batch_ms = W.stats_ms = 0.0;
  W.loaded = true;
  return LSSPA_OK;
}

// n = 0, (mean, M2) and the info word cleared
int mlift_reset(lsspa_ctx* ctx) {
  MultiLiftWork& W = ctx->mlift;
  return lift_stats_reset(ctx, W.st, (size_t)W.rf.m * W.rf.p, W.info, 8);
}

}  // namespace

extern "C" {

int lsspa_multi_lift_load(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* Y_train, int64_t ldy_train,
                          int64_t N, const void* X_test, int64_t ld_test, const void* Y_test, int64_t ldy_test,
                          int64_t M, int32_t p, int32_t m, double reg, int32_t dtype, int32_t location) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(mlift_limits(ctx, "lsspa_multi_lift_load", p, m));
  if (!multi_sides_ok(X_train, ld_train, Y_train, ldy_train, N, X_test, ld_test, Y_test, ldy_test, M, p, m, reg, dtype,
                      location))
    return ctx->fail(LSSPA_ERR_ARG, "lsspa_multi_lift_load: NULL array, N or M < 1, ld < p, ldy < m, reg not finite and "
                                    ">= 0, or bad dtype / location");
  if (M < p) {
    char msg[200];
    snprintf(msg, sizeof msg, "lsspa_multi_lift_load takes M >= p test rows (M = %lld, p = %d given): the test Gram "
             "matrix must have a Cholesky factor", (long long)M, (int)p);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  HIPCHK(hipSetDevice(ctx->device));
  MultiLiftWork& W = ctx->mlift;
  W.loaded = false;
  std::vector<double> G, g, H, h, yy;
  TRY(multi_reduce_sides(ctx, X_train, ld_train, Y_train, ldy_train, N, X_test, ld_test, Y_test, ldy_test, M, p, m, reg,
                         dtype, location, G, g, H, h, yy, W.gram_ms));
  return mlift_store(ctx, p, m, G.data(), g.data(), H.data(), h.data(), yy.data());
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_multi_lift_set_reduced(lsspa_ctx* ctx, int32_t p, int32_t m, const double* G, const double* g, const double* H,
                                 const double* h, const double* yy) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(mlift_limits(ctx, "lsspa_multi_lift_set_reduced", p, m));
  if (!G || !g || !H || !h || !yy) return ctx->fail(LSSPA_ERR_ARG, "lsspa_multi_lift_set_reduced: NULL array");
  HIPCHK(hipSetDevice(ctx->device));
  ctx->mlift.gram_ms = 0.0;
  return mlift_store(ctx, p, m, G, g, H, h, yy);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_multi_lift_set_players(lsspa_ctx* ctx, const int32_t* labels, int32_t g) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(mlift_need_loaded(ctx));
  MultiLiftWork& W = ctx->mlift;
  return lift_players_set(ctx, W.pl, "lsspa_multi_lift_set_players", W.rf.p, labels, g, [&] {
    HIPCHK(hipSetDevice(ctx->device));
    return mlift_reset(ctx);     // (waits for work in flight: a previous batch may still read the tables)
  });
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_multi_lift_batch(lsspa_ctx* ctx, const int32_t* perms, int64_t B, int32_t antithetical, double* lifts_out,
                           int32_t accumulate) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(mlift_need_loaded(ctx));
  MultiLiftWork& W = ctx->mlift;
  const int p = W.rf.p, m = W.rf.m, g = W.pl.ng, d = W.sd();
  // (with a map: two expanded rows a sample)
  TRY(lift_check_orderings(ctx, "lsspa_multi_lift_batch", "B", perms, B, p, g, d, g ? 2 : 1));
  HIPCHK(hipSetDevice(ctx->device));
  const int per = antithetical ? 2 : 1;
  const int64_t chunks = (m + MLIFT_RB - 1) / MLIFT_RB, entries = (int64_t)m * d;
  // samples a launch: by the grid and by the lift vectors' bytes -- by B, m, p and g alone
  const int64_t S = std::min(B, std::max<int64_t>(1, std::min(MLIFT_GRID_PER_LAUNCH / (per * chunks),
                                                              MLIFT_LIFT_DOUBLES / entries)));
  const int64_t rows_per = W.pl.rows_per(per);
  TRY(dev_alloc(ctx, W.lifts, (size_t)(S * entries)));
  TRY(dev_alloc(ctx, W.perms, (size_t)(S * rows_per * p)));
  LiftLaunchTimer t;
  TRY(t.create(ctx));
  W.batch_ms = W.stats_ms = 0.0;
  MultiLiftArgs a{};
  a.G = W.rf.G.ptr;
  a.H = W.rf.H.ptr;
  a.ld = p;
  a.g = W.rf.g.ptr;
  a.h = W.rf.h.ptr;
  a.yy = W.yy.ptr;
  a.aug[0] = W.aug[0];
  a.aug[1] = W.aug[1];
  a.perms = W.perms.ptr;
  a.p = p;
  a.nb = (p + MLIFT_RB + 15) / 16;
  a.per_sample = per;
  a.count = a.m = m;
  a.lifts = W.lifts.ptr;
  a.piv_tol = exact_piv_tol(p);
  a.info = W.info.ptr;
  a.ng = g;
  a.n_cols = g ? (int)W.pl.map.cols.size() : 0;
  a.off = W.pl.off();
  a.cols = W.pl.cols();
  for (int64_t s0 = 0; s0 < B; s0 += S) {
    const int64_t ns = std::min(S, B - s0);
    const int32_t* src = lift_stage_rows(W.pl.map, g, perms, s0, ns, per, p, W.pl.rows);
    HIPCHK(hipMemcpyAsync(W.perms.ptr, src, sizeof(int32_t) * (size_t)(ns * rows_per * p), hipMemcpyHostToDevice,
                          ctx->stream));
    if (per == 2)     // the pair's two terms are added into a zeroed destination
      HIPCHK(hipMemsetAsync(W.lifts.ptr, 0, sizeof(double) * (size_t)(ns * entries), ctx->stream));
    a.n_samples = (int)ns;
    TRY(t.mark(ctx, 0));
    HIPCHK(launch_multi_lift(a, ctx->stream));
    TRY(t.mark(ctx, 1));
    if (accumulate) TRY(lift_stats_fold(ctx, W.st, W.lifts.ptr, entries, ns));
    TRY(t.mark(ctx, 2));
    if (lifts_out)
      HIPCHK(hipMemcpyAsync(lifts_out + s0 * entries, W.lifts.ptr, sizeof(double) * (size_t)(ns * entries),
                            hipMemcpyDeviceToHost, ctx->stream));
    double lift_ms, fold_ms;
    TRY(t.finish(ctx, lift_ms, fold_ms));
    W.batch_ms += lift_ms;
    if (accumulate) W.stats_ms += fold_ms;
  }
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_multi_lift_get(lsspa_ctx* ctx, int64_t* n, double* mean, double* m2) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(mlift_need_loaded(ctx));
  const MultiLiftWork& W = ctx->mlift;
  return lift_stats_get(ctx, W.st, (size_t)W.rf.m * W.sd(), n, mean, m2);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_multi_lift_reset(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(mlift_need_loaded(ctx));
  HIPCHK(hipSetDevice(ctx->device));
  return mlift_reset(ctx);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_multi_lift_get_gram(lsspa_ctx* ctx, double* G, double* g, double* H, double* h, double* yy) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(mlift_need_loaded(ctx));
  reduced_get(ctx->mlift.rf, G, g, H, h, yy);
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_multi_lift_info(lsspa_ctx* ctx, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(mlift_need_loaded(ctx));
  if (!info) return ctx->fail(LSSPA_ERR_ARG, "lsspa_multi_lift_info: info is NULL");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpy(info, ctx->mlift.info.ptr, sizeof(int32_t), hipMemcpyDeviceToHost));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_multi_lift_timing(const lsspa_ctx* ctx, double* gram_ms, double* batch_ms, double* stats_ms) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (gram_ms) *gram_ms = ctx->mlift.gram_ms;
  if (batch_ms) *batch_ms = ctx->mlift.batch_ms;
  if (stats_ms) *stats_ms = ctx->mlift.stats_ms;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(const_cast<lsspa_ctx*>(ctx));
}

int lsspa_multi_lift_free(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->mlift.release();
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

}  // extern "C"

// ---- sampled attribution of the K-fold cross-validated R^2 (k_small.hip's fold launch, k_cv.hip) ----------------------
// The load packs the rows sorted by fold, runs the Gram reduction once per fold slice and finalises the K problems at the
// fold launch's stride.  A batch runs as launches of whole samples: the fold launch (grid (orderings, K)) writes
// raw [orderings][K][p], cv_lift_fold_kernel folds that to batch [samples][K + 1][d], launch_multi_lift_stats folds the
// samples into the running (n, mean, M2) [K + 1][d].
namespace {

constexpr int64_t CVLIFT_GRID_REG = 1 << 16;       // workgroups a launch of the register-resident form takes at most
constexpr int64_t CVLIFT_GRID_LDS = 1 << 13;       // ... of the LDS-resident form: one workgroup a compute unit, 32 rounds
constexpr int64_t CVLIFT_RAW_DOUBLES = (256ll << 20) / 8;     // raw lifts of a launch: 256 MB at most (one sample at least)

struct CvLiftPlan {
  int nb, form, threads;
  int64_t per_sample_wg, S, launches;
  size_t lds;
};

// the cut of a batch: a function of B, K, p and d alone (d does not enter: the raw lifts are p wide)
bool cvlift_plan(int64_t p, int64_t d, int64_t K, int64_t B, int antithetical, CvLiftPlan& P) {
  if (p < 1 || p > CV_LIFT_MAX_P || d < 1 || d > p || K < 2 || K > CV_MAX_FOLDS || B < 1) return false;
  const int64_t per = antithetical ? 2 : 1;
  P.nb = (int)((p + 1 + 15) / 16);
  P.form = P.nb <= 7 ? 0 : 1;
  P.threads = P.form ? 512 : 128;
  P.per_sample_wg = per * K;
  const int64_t cap = P.form ? CVLIFT_GRID_LDS : CVLIFT_GRID_REG;
  P.S = std::min(B, std::max<int64_t>(1, std::min(cap / (per * K), CVLIFT_RAW_DOUBLES / (per * K * p))));
  P.launches = (B + P.S - 1) / P.S;
  P.lds = small_folds_lds_bytes(P.nb);
  return true;
}

int cvlift_need_loaded(lsspa_ctx* ctx) {
  if (!ctx->cvlift.loaded)
    return ctx->fail(LSSPA_ERR_STATE, "no cross-validation data loaded for sampling (lsspa_cv_lift_load comes first)");
  return LSSPA_OK;
}

// n = 0, (mean, M2) and the info words cleared
int cvlift_reset(lsspa_ctx* ctx) {
  CvLiftWork& W = ctx->cvlift;
  return lift_stats_reset(ctx, W.st, (size_t)(W.K + 1) * W.p, W.info, CV_MAX_FOLDS);
}

}  // namespace

extern "C" {

int lsspa_cv_lift_load(lsspa_ctx* ctx, const void* X, int64_t ld, const void* y, int64_t N, int32_t p,
                       const int32_t* fold_ids, int32_t K, double reg, int32_t dtype, int32_t location) try {
  if (!ctx) return LSSPA_ERR_ARG;
  char msg[240];
  if (p > CV_LIFT_MAX_P) {
    snprintf(msg, sizeof msg, "lsspa_cv_lift_load takes at most p = %d features (%d given): both work matrices of an "
             "ordering, p + 1 rows each, stay in one workgroup", CV_LIFT_MAX_P, (int)p);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  if (K < 2 || K > CV_MAX_FOLDS) {
    snprintf(msg, sizeof msg, "cross-validation takes 2 .. %d folds (%d given)", CV_MAX_FOLDS, (int)K);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  if (!X || !y || !fold_ids || p < 1 || N < 2 || N >= (1ll << 31) || ld < p || !std::isfinite(reg) || reg < 0.0 ||
      (dtype != LSSPA_F64 && dtype != LSSPA_F32) || (location != LSSPA_HOST && location != LSSPA_DEVICE))
    return ctx->fail(LSSPA_ERR_ARG, "lsspa_cv_lift_load: NULL array, p < 1, N outside 2 .. 2^31 - 1, ld < p, reg not "
                                    "finite and >= 0, or bad dtype / location");
  int32_t nf[CV_MAX_FOLDS] = {0};
  if (cv_count_folds(fold_ids, N, K, nf, msg, sizeof msg)) return ctx->fail(LSSPA_ERR_ARG, msg);
  for (int f = 0; f < K; ++f)
    if (nf[f] < p) {
      snprintf(msg, sizeof msg, "fold %d of %d has %d rows, fewer than p = %d: the Gram matrix of a fold's own rows must "
               "have a Cholesky factor", f, (int)K, (int)nf[f], (int)p);
      return ctx->fail(LSSPA_ERR_ARG, msg);
    }
  // (rows on the device: the pooled sum is looked at after the Gram passes)
  if (location == LSSPA_HOST && host_all_zero(y, N, dtype))
    return ctx->fail(LSSPA_ERR_ARG, "y is identically zero (sum y^2 = 0): the cross-validated R^2 is not defined");
  HIPCHK(hipSetDevice(ctx->device));
  CvLiftWork& W = ctx->cvlift;
  W.loaded = false;
  W.pl.ng = 0;              // a player map belongs to the data it was set on
  hipStream_t st = ctx->stream;
  // every row's place when the rows are sorted by fold, stable in row order
  std::vector<int32_t> dest((size_t)N);
  int64_t first[CV_MAX_FOLDS + 1] = {0};
  for (int f = 0; f < K; ++f) first[f + 1] = first[f] + nf[f];
  {
    int64_t at[CV_MAX_FOLDS];
    std::copy(first, first + K, at);
    for (int64_t i = 0; i < N; ++i) dest[(size_t)i] = (int32_t)at[fold_ids[i]]++;
  }
  constexpr size_t LD = CV_LIFT_LD, LL = LD * LD;
  DevBuf<double> Xs, ys, S;
  DevBuf<int32_t> dst_d, nf_d;
  DevBuf<char> stage_x, stage_y;
  struct Scratch {
    DevBuf<double>&a, &b, &c;
    DevBuf<int32_t>&d, &e;
    DevBuf<char>&f, &g;
    ~Scratch() { dev_free(a); dev_free(b); dev_free(c); dev_free(d); dev_free(e); dev_free(f); dev_free(g); }
  } scratch{Xs, ys, S, dst_d, nf_d, stage_x, stage_y};
  TRY(dev_alloc(ctx, Xs, (size_t)N * LD));
  TRY(dev_alloc(ctx, ys, (size_t)N));
  TRY(dev_alloc(ctx, S, (size_t)K * LL));
  TRY(dev_alloc(ctx, dst_d, (size_t)N));
  TRY(dev_alloc(ctx, nf_d, CV_MAX_FOLDS));
  TRY(lift_problems_alloc(ctx, W.pr, (size_t)K, CV_MAX_FOLDS));
  TRY(dev_alloc(ctx, W.info, CV_MAX_FOLDS));
  TRY(lift_stats_alloc(ctx, W.st, (size_t)(K + 1) * p));
  HIPCHK(hipStreamSynchronize(st));      // a previous call may still read the buffers
  HIPCHK(hipMemcpy(dst_d.ptr, dest.data(), sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(nf_d.ptr, nf, sizeof nf, hipMemcpyHostToDevice));
  TRY(lift_problems_zero(ctx, W.pr, (size_t)K, st));
  std::vector<hipEvent_t> ev(2, nullptr);
  Events guard{ev};
  for (hipEvent_t& e : ev) HIPCHK(hipEventCreate(&e));
  HIPCHK(hipEventRecord(ev[0], st));
  TRY(load_rows(ctx, stage_x, stage_y, X, ld, y, N, p, dtype, location,
                [&](const void* sx, const void* sy, int64_t nr, int64_t r0) {
                  return launch_cv_lift_pack(sx, ld, sy, nr, p, dtype == LSSPA_F32, dst_d.ptr + r0, Xs.ptr, ys.ptr, st);
                }));
  for (int f = 0; f < K; ++f)            // S_f: the Gram reduction on the fold's slice (gram_side waits for it)
    TRY(gram_side(ctx, Xs.ptr + (size_t)first[f] * LD, ys.ptr + first[f], nf[f], (int64_t)LD, p, 0, S.ptr + (size_t)f * LL));
  HIPCHK(launch_cv_lift_finalize(S.ptr, nf_d.ptr, N, p, K, reg, W.pr.G.ptr, W.pr.g.ptr, W.pr.H.ptr, W.pr.h.ptr,
                                 W.pr.inv_yy.ptr, W.pr.aug.ptr, st));
  HIPCHK(hipEventRecord(ev[1], st));
  const size_t pp = (size_t)p * p;
  W.Gh.resize(K * pp);
  W.Hh.resize(K * pp);
  W.gh.resize((size_t)K * p);
  W.hh.resize((size_t)K * p);
  W.yh.resize((size_t)K);
  TRY(lift_problems_copy_out(ctx, W.pr, 0, K, p, W.Gh.data(), W.Hh.data(), W.gh.data(), W.hh.data(), W.yh.data(), st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
  W.gram_ms = ms;
  W.batch_ms = W.stats_ms = 0.0;
  if (!(W.yh[0] > 0.0) || !std::isfinite(W.yh[0]))
    return ctx->fail(LSSPA_ERR_ARG, "y is identically zero (sum y^2 = 0): the cross-validated R^2 is not defined");
  W.p = p;
  W.K = K;
  TRY(lift_stats_clear(ctx, W.st, (size_t)(K + 1) * p));
  HIPCHK(hipMemset(W.info.ptr, 0, sizeof(int32_t) * CV_MAX_FOLDS));
  W.loaded = true;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_cv_lift_set_players(lsspa_ctx* ctx, const int32_t* labels, int32_t g) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(cvlift_need_loaded(ctx));
  CvLiftWork& W = ctx->cvlift;
  return lift_players_set(ctx, W.pl, "lsspa_cv_lift_set_players", W.p, labels, g, [&] {
    HIPCHK(hipSetDevice(ctx->device));
    return cvlift_reset(ctx);    // (waits for work in flight: a previous batch may still read the tables)
  });
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_cv_lift_batch(lsspa_ctx* ctx, const int32_t* perms, int64_t B, int32_t antithetical, double* fold_lifts_out,
                        double* lifts_out, int32_t accumulate) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(cvlift_need_loaded(ctx));
  CvLiftWork& W = ctx->cvlift;
  const int p = W.p, K = W.K, g = W.pl.ng, d = W.sd();
  TRY(lift_check_orderings(ctx, "lsspa_cv_lift_batch", "B", perms, B, p, g, d, 2));
  HIPCHK(hipSetDevice(ctx->device));
  const int per = antithetical ? 2 : 1;
  CvLiftPlan P;
  if (!cvlift_plan(p, d, K, B, antithetical, P)) return ctx->fail(LSSPA_ERR_ARG, "lsspa_cv_lift_batch: no launch plan");
  const int64_t S = P.S, entries = (int64_t)(K + 1) * d;
  const int64_t rows_per = W.pl.rows_per(per);
  TRY(dev_alloc(ctx, W.raw, (size_t)(S * per * K * p)));
  TRY(dev_alloc(ctx, W.batch, (size_t)(S * entries)));
  TRY(dev_alloc(ctx, W.perms, (size_t)(S * rows_per * p)));
  LiftLaunchTimer t;
  TRY(t.create(ctx));
  W.batch_ms = W.stats_ms = 0.0;
  SmallArgs a = lift_small_args(p, P.nb, per, g, W.raw.ptr);
  SmallFolds fo{};
  lift_problems_args(W.pr, 0, K, a, fo);
  a.perms = W.perms.ptr;
  a.info = W.info.ptr;
  for (int64_t s0 = 0; s0 < B; s0 += S) {
    const int64_t ns = std::min(S, B - s0);
    const int32_t* src = lift_stage_rows(W.pl.map, g, perms, s0, ns, per, p, W.pl.rows);
    HIPCHK(hipMemcpyAsync(W.perms.ptr, src, sizeof(int32_t) * (size_t)(ns * rows_per * p), hipMemcpyHostToDevice,
                          ctx->stream));
    a.n_ord = (int)(ns * per);
    TRY(t.mark(ctx, 0));
    HIPCHK(launch_small_folds(a, fo, ctx->stream));
    TRY(t.mark(ctx, 1));
    HIPCHK(launch_cv_lift_fold(W.raw.ptr, p, K, per, W.pl.off(), W.pl.cols(), d, ns, W.batch.ptr, ctx->stream));
    if (accumulate) TRY(lift_stats_fold(ctx, W.st, W.batch.ptr, entries, ns));
    TRY(t.mark(ctx, 2));
    if (fold_lifts_out)
      HIPCHK(hipMemcpy2DAsync(fold_lifts_out + s0 * K * d, sizeof(double) * K * d, W.batch.ptr, sizeof(double) * entries,
                              sizeof(double) * K * d, (size_t)ns, hipMemcpyDeviceToHost, ctx->stream));
    if (lifts_out)
      HIPCHK(hipMemcpy2DAsync(lifts_out + s0 * d, sizeof(double) * d, W.batch.ptr + (size_t)K * d,
                              sizeof(double) * entries, sizeof(double) * d, (size_t)ns, hipMemcpyDeviceToHost,
                              ctx->stream));
    double lift_ms, fold_ms;
    TRY(t.finish(ctx, lift_ms, fold_ms));
    W.batch_ms += lift_ms;
    W.stats_ms += fold_ms;
  }
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_cv_lift_get(lsspa_ctx* ctx, int64_t* n, double* mean, double* m2) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(cvlift_need_loaded(ctx));
  const CvLiftWork& W = ctx->cvlift;
  return lift_stats_get(ctx, W.st, (size_t)(W.K + 1) * W.sd(), n, mean, m2);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_cv_lift_reset(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(cvlift_need_loaded(ctx));
  HIPCHK(hipSetDevice(ctx->device));
  return cvlift_reset(ctx);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_cv_lift_get_problem(lsspa_ctx* ctx, int32_t f, double* G, double* g, double* H, double* h, double* inv_yy) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(cvlift_need_loaded(ctx));
  const CvLiftWork& W = ctx->cvlift;
  if (f < 0 || f >= W.K) return ctx->fail(LSSPA_ERR_ARG, "lsspa_cv_lift_get_problem: f must be 0 .. K - 1");
  const size_t p = (size_t)W.p, pp = p * p;
  if (G) std::copy(W.Gh.begin() + f * pp, W.Gh.begin() + (f + 1) * pp, G);
  if (H) std::copy(W.Hh.begin() + f * pp, W.Hh.begin() + (f + 1) * pp, H);
  if (g) std::copy(W.gh.begin() + f * p, W.gh.begin() + (f + 1) * p, g);
  if (h) std::copy(W.hh.begin() + f * p, W.hh.begin() + (f + 1) * p, h);
  if (inv_yy) *inv_yy = W.yh[(size_t)f];
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_cv_lift_info(lsspa_ctx* ctx, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(cvlift_need_loaded(ctx));
  if (!info) return ctx->fail(LSSPA_ERR_ARG, "lsspa_cv_lift_info: info is NULL");
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipMemcpy(info, ctx->cvlift.info.ptr, sizeof(int32_t) * ctx->cvlift.K, hipMemcpyDeviceToHost));
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_cv_lift_timing(const lsspa_ctx* ctx, double* gram_ms, double* batch_ms, double* stats_ms) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (gram_ms) *gram_ms = ctx->cvlift.gram_ms;
  if (batch_ms) *batch_ms = ctx->cvlift.batch_ms;
  if (stats_ms) *stats_ms = ctx->cvlift.stats_ms;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(const_cast<lsspa_ctx*>(ctx));
}

int lsspa_cv_lift_free(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->cvlift.release();
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_cv_lift_plan(int32_t p, int32_t d, int32_t K, int64_t B, int32_t antithetical, int64_t* plan) {
  CvLiftPlan P;
  if (!plan || !cvlift_plan(p, d, K, B, antithetical, P)) return LSSPA_ERR_ARG;
  plan[0] = P.nb;
  plan[1] = P.form;
  plan[2] = P.per_sample_wg;
  plan[3] = P.S;
  plan[4] = P.launches;
  plan[5] = (int64_t)P.lds;
  plan[6] = P.threads;
  plan[7] = 0;
  return LSSPA_OK;
}

}  // extern "C"

// ---- bootstrap of the sampled attribution (k_boot.hip's wide Gram pass, launch_small_problems) -------------------------
// The rows of both sides stay on the device as Z = [X | y] (ldz = 16 cb, cb <= 8); the orderings are set once and shared
// by every replicate and the point problem.  A run goes block by block (boot_lift_plan): weights, the weighted Grams and
// their sums, finalise into the ordering kernels' layout, then lift launches with the grid (orderings, replicates) --
// cut into samples_per_launch samples and reps_per_launch replicates -- each followed by boot_lift_stats_kernel's merge
// into the replicates' running (mean, M2).
namespace {

int bootlift_need_loaded(lsspa_ctx* ctx) {
  if (!ctx->bootlift.loaded)
    return ctx->fail(LSSPA_ERR_STATE, "no bootstrap data loaded for sampling (lsspa_boot_lift_load comes first)");
  return LSSPA_OK;
}

// what a pass over replicates leaves with the caller; any pointer may be NULL
struct BootLiftOut {
  double *mean = nullptr, *m2 = nullptr, *r2 = nullptr, *base = nullptr, *samples = nullptr;
  int32_t* info = nullptr;
  double *G = nullptr, *g = nullptr, *H = nullptr, *h = nullptr, *inv_yy = nullptr;      // of the pass's first replicate
  double *S_train = nullptr, *S_test = nullptr, *wsum = nullptr;                          // before finalise
  bool lifts = false;               // run the orderings (else the Gram side only)
};

// Replicates first .. first + R - 1: a side's weights are the caller's rows w_host[s] [R][n], or ones, or the counts of
// (seed, replicate, side).
int bootlift_pass(lsspa_ctx* ctx, const char* name, int64_t R, uint64_t seed, int64_t first, const double* const w_host[2],
                  bool ones, int64_t block, const BootLiftOut& out) {
  BootLiftWork& B = ctx->bootlift;
  const int p = B.p, d = B.sd(), c = p + 1;
  constexpr int64_t LD = LiftProblems::LD, LL = LiftProblems::LL;
  const int per = out.lifts ? B.per : 1;
  const int64_t n_samples = out.lifts ? B.n_samples : 1;
  BootLiftPlan P;
  if (const char* why = boot_lift_plan(R, B.n[0], B.n[1], p, d, n_samples, per == 2, block, P)) {
    char msg[240];
    snprintf(msg, sizeof msg, "%s: %s", name, why);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  if (w_host[0]) TRY(boot_check_weights(ctx, w_host[0], R, B.n[0], "w_train"));
  if (w_host[1]) TRY(boot_check_weights(ctx, w_host[1], R, B.n[1], "w_test"));
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t blk = (size_t)P.block, cc = (size_t)c * c;
  for (int s = 0; s < 2; ++s) {
    if (!w_host[s] && !ones)
      TRY(dev_alloc(ctx, B.cnt(s), blk * (size_t)B.n[s]));
    else
      TRY(dev_alloc(ctx, B.wt(s), blk * (size_t)B.n[s]));
    TRY(dev_alloc(ctx, B.part(s), (size_t)P.slices[s] * blk * P.pairs * 256));
    TRY(dev_alloc(ctx, B.S(s), blk * cc));
  }
  TRY(dev_alloc(ctx, B.wsum, blk));
  TRY(lift_problems_alloc(ctx, B.pr, blk, blk));
  TRY(dev_alloc(ctx, B.info, blk));
  const int64_t E = std::min<int64_t>(P.reps_per_launch, P.block), S = P.samples_per_launch;
  if (out.lifts) {
    TRY(dev_alloc(ctx, B.raw, (size_t)(S * per * E * p)));
    TRY(dev_alloc(ctx, B.mean, blk * d));
    TRY(dev_alloc(ctx, B.M2, blk * d));
    if (out.samples) TRY(dev_alloc(ctx, B.samples, (size_t)(E * S * d)));
  }
  HIPCHK(hipStreamSynchronize(st));        // a previous call may still read the buffers
  TRY(lift_problems_zero(ctx, B.pr, blk, st));
  const int64_t cuts = P.sample_cuts, per_block = (P.block + E - 1) / E * cuts;
  std::vector<hipEvent_t> ev((size_t)(3 + (out.lifts ? 2 * per_block : 0)), nullptr);
  Events guard{ev};
  for (hipEvent_t& e : ev) HIPCHK(hipEventCreate(&e));
  const int g = B.pl.ng;
  const int64_t rows_per = B.pl.rows_per(per);
  SmallArgs a = lift_small_args(p, P.cb, per, g, B.raw.ptr);
  SmallFolds fo{};
  std::vector<double> one, Gh, Hh, gh, hh, yh, ws;
  std::vector<int> all((size_t)p), basec;
  for (int j = 0; j < p; ++j) all[(size_t)j] = j;
  if (g) basec.assign(B.pl.map.base.begin(), B.pl.map.base.end());
  constexpr int CH = 32;                     // replicates whose problems come to the host at a time (their R^2)
  if (out.r2 || out.base) {
    Gh.resize((size_t)CH * LD * p);
    Hh.resize((size_t)CH * LD * p);
    gh.resize((size_t)CH * p);
    hh.resize((size_t)CH * p);
    yh.resize(CH);
  }
  B.ms[0] = B.ms[1] = B.ms[2] = B.ms[3] = 0.0;
  B.launches = 0;
  for (int64_t b0 = 0; b0 < R; b0 += P.block) {
    const int nb = (int)std::min<int64_t>(P.block, R - b0);
    HIPCHK(hipEventRecord(ev[0], st));
    for (int s = 0; s < 2; ++s) {
      if (w_host[s]) {
        HIPCHK(hipMemcpyAsync(B.wt(s).ptr, w_host[s] + b0 * B.n[s], sizeof(double) * (size_t)nb * B.n[s],
                              hipMemcpyHostToDevice, st));
      } else if (ones) {
        one.assign((size_t)nb * B.n[s], 1.0);
        HIPCHK(hipMemcpyAsync(B.wt(s).ptr, one.data(), sizeof(double) * one.size(), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));        // `one` is reused for the other side
      } else {
        HIPCHK(launch_boot_counts(seed, (uint64_t)first + (uint64_t)b0, s, B.n[s], nb, B.cnt(s).ptr, st));
      }
    }
    HIPCHK(hipEventRecord(ev[1], st));
    for (int s = 0; s < 2; ++s) {
      const bool counts = !w_host[s] && !ones;
      const uint32_t* cnt = counts ? B.cnt(s).ptr : nullptr;
      const double* wt = counts ? nullptr : B.wt(s).ptr;
      HIPCHK(launch_boot_lift_gram(P, s, B.Z(s).ptr, B.n[s], cnt, wt, nb, B.part(s).ptr, st));
      if (s == 0) HIPCHK(launch_boot_wsum(cnt, wt, B.n[s], nb, B.wsum.ptr, st));
      HIPCHK(launch_boot_lift_reduce(P, s, B.part(s).ptr, p, nb, B.S(s).ptr, st));
    }
    HIPCHK(launch_boot_lift_finalize(B.S0.ptr, B.S1.ptr, B.wsum.ptr, p, B.reg, nb, B.pr.G.ptr, B.pr.g.ptr, B.pr.H.ptr,
                                     B.pr.h.ptr, B.pr.inv_yy.ptr, B.pr.aug.ptr, st));
    HIPCHK(hipEventRecord(ev[2], st));
    HIPCHK(hipMemsetAsync(B.info.ptr, 0, sizeof(int32_t) * nb, st));
    size_t ne = 3;
    if (out.lifts) {
      for (int64_t e0 = 0; e0 < nb; e0 += E) {
        const int nr = (int)std::min<int64_t>(E, nb - e0);
        lift_problems_args(B.pr, e0, nr, a, fo);
        a.info = B.info.ptr + e0;
        for (int64_t s0 = 0; s0 < n_samples; s0 += S) {
          const int ns = (int)std::min<int64_t>(S, n_samples - s0);
          a.perms = B.perms.ptr + s0 * rows_per * p;
          a.n_ord = ns * per;
          HIPCHK(launch_small_problems(a, fo, st));
          HIPCHK(hipEventRecord(ev[ne++], st));
          HIPCHK(launch_boot_lift_stats(B.raw.ptr, p, nr, per, B.pl.off(), B.pl.cols(), d, ns, s0, B.mean.ptr + e0 * d,
                                        B.M2.ptr + e0 * d, out.samples ? B.samples.ptr : nullptr, st));
          HIPCHK(hipEventRecord(ev[ne++], st));
          if (out.samples)
            HIPCHK(hipMemcpy2DAsync(out.samples + ((b0 + e0) * n_samples + s0) * d, sizeof(double) * n_samples * d,
                                    B.samples.ptr, sizeof(double) * ns * d, sizeof(double) * ns * d, (size_t)nr,
                                    hipMemcpyDeviceToHost, st));
          ++B.launches;
        }
      }
      if (out.mean)
        HIPCHK(hipMemcpyAsync(out.mean + b0 * d, B.mean.ptr, sizeof(double) * (size_t)nb * d, hipMemcpyDeviceToHost, st));
      if (out.m2)
        HIPCHK(hipMemcpyAsync(out.m2 + b0 * d, B.M2.ptr, sizeof(double) * (size_t)nb * d, hipMemcpyDeviceToHost, st));
    }
    if (out.info) HIPCHK(hipMemcpyAsync(out.info + b0, B.info.ptr, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, st));
    if (out.S_train)
      HIPCHK(hipMemcpyAsync(out.S_train + b0 * cc, B.S0.ptr, sizeof(double) * nb * cc, hipMemcpyDeviceToHost, st));
    if (out.S_test)
      HIPCHK(hipMemcpyAsync(out.S_test + b0 * cc, B.S1.ptr, sizeof(double) * nb * cc, hipMemcpyDeviceToHost, st));
    if (out.wsum) HIPCHK(hipMemcpyAsync(out.wsum + b0, B.wsum.ptr, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
    if (b0 == 0) TRY(lift_problems_copy_out(ctx, B.pr, 0, 1, p, out.G, out.H, out.g, out.h, out.inv_yy, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int k = 0; k < 2; ++k) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
      B.ms[k] += ms;
    }
    for (size_t k = 2; k + 1 < ne; ++k) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
      B.ms[2 + (k & 1)] += ms;             // ev[2] -> ev[3]: a lift launch; ev[3] -> ev[4]: its statistics; ...
    }
    if (out.r2 || out.base)                // R^2 of the full model and of the baseline's columns, on the host
      for (int c0 = 0; c0 < nb; c0 += CH) {
        const int nc = std::min(CH, nb - c0);
        const size_t w = sizeof(double) * p;
        // (a chunk's matrices in one copy each, the padding rows with them: not lift_problems_copy_out's dense form)
        HIPCHK(hipMemcpy2D(Gh.data(), w, B.pr.G.ptr + c0 * LL, sizeof(double) * LD, w, (size_t)nc * LD, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy2D(Hh.data(), w, B.pr.H.ptr + c0 * LL, sizeof(double) * LD, w, (size_t)nc * LD, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy2D(gh.data(), w, B.pr.g.ptr + c0 * LD, sizeof(double) * LD, w, (size_t)nc, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy2D(hh.data(), w, B.pr.h.ptr + c0 * LD, sizeof(double) * LD, w, (size_t)nc, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(yh.data(), B.pr.inv_yy.ptr + c0, sizeof(double) * nc, hipMemcpyDeviceToHost));
        for (int r = 0; r < nc; ++r) {
          const double *Gr = &Gh[(size_t)r * LD * p], *Hr = &Hh[(size_t)r * LD * p];
          const double *gr = &gh[(size_t)r * p], *hr = &hh[(size_t)r * p];
          if (out.r2) out.r2[b0 + c0 + r] = boot_r2_cols(p, all.data(), p, Gr, gr, Hr, hr, yh[(size_t)r], ws);
          if (out.base)
            out.base[b0 + c0 + r] = boot_r2_cols(p, basec.data(), (int)basec.size(), Gr, gr, Hr, hr, yh[(size_t)r], ws);
        }
      }
  }
  return LSSPA_OK;
}

}  // namespace

extern "C" {

int lsspa_boot_lift_load(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* y_train, int64_t N,
                         const void* X_test, int64_t ld_test, const void* y_test, int64_t M, int32_t p, double reg,
                         int32_t dtype, int32_t location) try {
  if (!ctx) return LSSPA_ERR_ARG;
  char msg[240];
  if (p > BOOT_LIFT_MAX_P) {
    snprintf(msg, sizeof msg, "lsspa_boot_lift_load takes at most p = %d features (%d given): both work matrices of an "
             "ordering, p + 1 rows each, stay in one workgroup", BOOT_LIFT_MAX_P, (int)p);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  BootLiftPlan P;
  if (const char* why = boot_lift_plan(1, N, M, p, p < 1 ? 1 : p, 1, 0, 0, P)) {
    snprintf(msg, sizeof msg, "lsspa_boot_lift_load: %s", why);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  if (N < p || M < p) {
    snprintf(msg, sizeof msg, "lsspa_boot_lift_load: N = %lld and M = %lld rows must both be at least p = %d (the Gram "
             "matrices of both sides must have a Cholesky factor)", (long long)N, (long long)M, (int)p);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  if (!X_train || !y_train || !X_test || !y_test || ld_train < p || ld_test < p || !std::isfinite(reg) || reg < 0.0 ||
      (dtype != LSSPA_F64 && dtype != LSSPA_F32) || (location != LSSPA_HOST && location != LSSPA_DEVICE))
    return ctx->fail(LSSPA_ERR_ARG, "lsspa_boot_lift_load: NULL array, ld < p, reg not finite and >= 0, or bad dtype / "
                                    "location");
  if (location == LSSPA_HOST && host_all_zero(y_test, M, dtype))
    return ctx->fail(LSSPA_ERR_ARG, "y_test is identically zero (sum y^2 = 0): R^2 is not defined");
  HIPCHK(hipSetDevice(ctx->device));
  BootLiftWork& B = ctx->bootlift;
  B.loaded = false;
  B.pl.ng = 0;              // a player map and the orderings belong to the data they were set on
  B.n_samples = 0;
  const void* X[2] = {X_train, X_test};
  const void* y[2] = {y_train, y_test};
  const int64_t n[2] = {N, M}, ld[2] = {ld_train, ld_test};
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (int s = 0; s < 2; ++s) {
    TRY(dev_alloc(ctx, B.Z(s), (size_t)n[s] * P.ldz));
    TRY(load_rows(ctx, B.stage_x, B.stage_y, X[s], ld[s], y[s], n[s], p, dtype, location,
                  [&](const void* sx, const void* sy, int64_t nr, int64_t r0) {
                    return launch_boot_lift_pack(sx, ld[s], sy, nr, p, dtype == LSSPA_F32, B.Z(s).ptr, P.ldz, r0,
                                                 ctx->stream);
                  }));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  dev_free(B.stage_x);
  dev_free(B.stage_y);
  B.p = p;
  B.n[0] = N;
  B.n[1] = M;
  B.reg = reg;
  B.ms[0] = B.ms[1] = B.ms[2] = B.ms[3] = 0.0;
  B.loaded = true;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_boot_lift_set_players(lsspa_ctx* ctx, const int32_t* labels, int32_t g) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(bootlift_need_loaded(ctx));
  BootLiftWork& B = ctx->bootlift;
  return lift_players_set(ctx, B.pl, "lsspa_boot_lift_set_players", B.p, labels, g, [&] {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));      // a previous run may still read the tables
    B.n_samples = 0;                                // the orderings were orderings of the other players
    return (int)LSSPA_OK;
  });
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_boot_lift_set_orderings(lsspa_ctx* ctx, const int32_t* perms, int64_t n_samples, int32_t antithetical) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(bootlift_need_loaded(ctx));
  BootLiftWork& B = ctx->bootlift;
  const int p = B.p, g = B.pl.ng, d = B.sd();
  TRY(lift_check_orderings(ctx, "lsspa_boot_lift_set_orderings", "n_samples", perms, n_samples, p, g, d, 2));
  HIPCHK(hipSetDevice(ctx->device));
  const int per = antithetical ? 2 : 1;
  const int64_t rows_per = B.pl.rows_per(per);
  HIPCHK(hipStreamSynchronize(ctx->stream));      // a previous run may still read the rows
  B.n_samples = 0;
  TRY(dev_alloc(ctx, B.perms, (size_t)(n_samples * rows_per * p)));
  std::vector<int32_t> rows;     // (all the samples at once: not kept)
  const int32_t* src = lift_stage_rows(B.pl.map, g, perms, 0, n_samples, per, p, rows);
  HIPCHK(hipMemcpy(B.perms.ptr, src, sizeof(int32_t) * (size_t)(n_samples * rows_per * p), hipMemcpyHostToDevice));
  B.n_samples = n_samples;
  B.per = per;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_boot_lift_run(lsspa_ctx* ctx, int64_t R, uint64_t boot_seed, int64_t first, const double* w_train,
                        const double* w_test, int64_t block, double* mean, double* m2, double* r2, double* baseline_r2,
                        int32_t* info, double* samples_out) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(bootlift_need_loaded(ctx));
  if (ctx->bootlift.n_samples < 1)
    return ctx->fail(LSSPA_ERR_STATE, "no orderings set (lsspa_boot_lift_set_orderings comes first)");
  if (!mean || !m2 || !r2 || !info || first < 0)
    return ctx->fail(LSSPA_ERR_ARG, "lsspa_boot_lift_run: mean / m2 / r2 / info NULL or first < 0");
  BootLiftOut out;
  out.mean = mean;
  out.m2 = m2;
  out.r2 = r2;
  out.base = baseline_r2;
  out.info = info;
  out.samples = samples_out;
  out.lifts = true;
  const double* const w[2] = {w_train, w_test};
  return bootlift_pass(ctx, "lsspa_boot_lift_run", R, boot_seed, first, w, false, block, out);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_boot_lift_point(lsspa_ctx* ctx, double* mean, double* m2, double* r2, double* baseline_r2, int32_t* info,
                          double* samples_out) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(bootlift_need_loaded(ctx));
  if (ctx->bootlift.n_samples < 1)
    return ctx->fail(LSSPA_ERR_STATE, "no orderings set (lsspa_boot_lift_set_orderings comes first)");
  if (!mean || !m2 || !r2 || !info) return ctx->fail(LSSPA_ERR_ARG, "lsspa_boot_lift_point: mean / m2 / r2 / info NULL");
  BootLiftOut out;
  out.mean = mean;
  out.m2 = m2;
  out.r2 = r2;
  out.base = baseline_r2;
  out.info = info;
  out.samples = samples_out;
  out.lifts = true;
  const double* const w[2] = {nullptr, nullptr};
  return bootlift_pass(ctx, "lsspa_boot_lift_point", 1, 0, 0, w, true, 1, out);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_boot_lift_get_problem(lsspa_ctx* ctx, int64_t r, uint64_t boot_seed, const double* w_train, const double* w_test,
                                double* G, double* g, double* H, double* h, double* inv_yy) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(bootlift_need_loaded(ctx));
  BootLiftOut out;
  out.G = G;
  out.g = g;
  out.H = H;
  out.h = h;
  out.inv_yy = inv_yy;
  const double* const w[2] = {w_train, w_test};
  // r < 0: the point problem, weight 1 on every row of a side without weights
  return bootlift_pass(ctx, "lsspa_boot_lift_get_problem", 1, boot_seed, r < 0 ? 0 : r, w, r < 0, 1, out);
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_boot_lift_debug_grams(lsspa_ctx* ctx, int64_t R, const double* w_train, const double* w_test, double* S_train,
                                double* S_test, double* wsum) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(bootlift_need_loaded(ctx));
  BootLiftOut out;
  out.S_train = S_train;
  out.S_test = S_test;
  out.wsum = wsum;
  const double* const w[2] = {w_train, w_test};
  return bootlift_pass(ctx, "lsspa_boot_lift_debug_grams", R, 0, 0, w, true, 0, out);   // no weights: ones, not counts
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_boot_lift_timing(const lsspa_ctx* ctx, double* counts_ms, double* gram_ms, double* lift_ms, double* stats_ms,
                           int64_t* launches) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (counts_ms) *counts_ms = ctx->bootlift.ms[0];
  if (gram_ms) *gram_ms = ctx->bootlift.ms[1];
  if (lift_ms) *lift_ms = ctx->bootlift.ms[2];
  if (stats_ms) *stats_ms = ctx->bootlift.ms[3];
  if (launches) *launches = ctx->bootlift.launches;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(const_cast<lsspa_ctx*>(ctx));
}

int lsspa_boot_lift_free(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->bootlift.release();
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_debug_boot_lift_plan(int64_t R, int64_t N, int64_t M, int32_t p, int32_t d, int64_t n_samples,
                               int32_t antithetical, int64_t block, int64_t* plan16) try {
  BootLiftPlan P;
  if (!plan16 || boot_lift_plan(R, N, M, p, d, n_samples, antithetical, block, P)) return LSSPA_ERR_ARG;
  const int64_t v[16] = {P.cb, P.gram_form, P.rps[0], P.rps[1], P.slices[0], P.slices[1], P.block, P.n_blocks,
                         P.reps_per_launch, P.ord_per_launch, P.samples_per_launch, P.sample_cuts, P.launches,
                         P.raw_bytes, P.lift_form, P.rep_bytes};
  std::copy(v, v + 16, plan16);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_NOMEM;
}

}  // extern "C"

// ---- permutation test of the exact attribution (k_perm.hip, host_perms.cpp) -------------------------------------------
// G, H and ||y_test||^2 do not depend on a permutation of y: one Gram pass per side over [X | y] at the load gives them
// and the observed g, h.  A run then goes block by block: the index rows of a block's replicates are drawn by threads of
// this library into pinned memory and uploaded on a stream of their own while the GPU works on the block before; one
// gathered X^T y pass per permuted side and a fixed-order sum over its slices write g_r, h_r into the response slots of
// the PermWork's own MultiWork, which the enumerations of lsspa_multi_shapley / lsspa_multi_groups_shapley then read.
namespace {

int perm_need_loaded(lsspa_ctx* ctx) {
  if (!ctx->perm.loaded) return ctx->fail(LSSPA_ERR_STATE, "no permutation-test data loaded (lsspa_perm_load comes first)");
  return LSSPA_OK;
}

// labels / g of a run against the loaded columns, before any GPU work
int perm_players(lsspa_ctx* ctx, const char* name, const int32_t* labels, int32_t g) {
  const int p = ctx->perm.p;
  char msg[240];
  if (!labels) {
    if (p > MULTI_MAX_P) {
      snprintf(msg, sizeof msg, "%s enumerates all 2^p feature subsets and takes at most p = %d features without labels "
               "(%d loaded); with labels it attributes to groups of up to %d columns", name, MULTI_MAX_P, p, GROUPS_MAX_P);
      return ctx->fail(LSSPA_ERR_ARG, msg);
    }
    return LSSPA_OK;
  }
  if (g > GROUPS_MAX_G) {
    snprintf(msg, sizeof msg, "exact attribution over groups takes at most g = %d groups (%d given)", GROUPS_MAX_G, (int)g);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  GroupLayout L;
  if (const char* why = groups_layout(labels, p, g, L)) {
    snprintf(msg, sizeof msg, "group labels: %s", why);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  return LSSPA_OK;
}

// response slots for `cap` replicates: g, h [cap][p] and inv_yy [cap] = 1 / ||y_test||^2 (a permutation leaves it)
int perm_slots(lsspa_ctx* ctx, int64_t cap) {
  PermWork& W = ctx->perm;
  MultiWork& Mw = W.mw;
  TRY(dev_alloc(ctx, Mw.rf.g, (size_t)cap * W.p));
  TRY(dev_alloc(ctx, Mw.rf.h, (size_t)cap * W.p));
  TRY(dev_alloc(ctx, Mw.inv_yy, (size_t)cap));
  std::vector<double> inv((size_t)cap, 1.0 / Mw.rf.yyh[0]);
  HIPCHK(hipStreamSynchronize(ctx->stream));     // a previous call may still read the slots
  HIPCHK(hipMemcpy(Mw.inv_yy.ptr, inv.data(), sizeof(double) * (size_t)cap, hipMemcpyHostToDevice));
  return LSSPA_OK;
}

int perm_enumerate(lsspa_ctx* ctx, const int32_t* labels, int32_t g, int64_t count, double* phi, int32_t* bits) {
  MultiWork& Mw = ctx->perm.mw;
  Mw.rf.m = (int)count;
  return labels ? multi_groups_shapley_on(ctx, Mw, labels, g, 0, count, 0, phi, bits)
                : multi_shapley_on(ctx, Mw, 0, count, 0, phi, bits);
}

// the producer of one block's index rows: a thread of this library that draws into pinned memory and uploads on `up`
struct PermProducer {
  std::thread th;
  hipError_t err = hipSuccess;
  double draw_ms = 0.0, upload_ms = 0.0;
  ~PermProducer() {
    if (th.joinable()) th.join();
  }
  void wait() {
    if (th.joinable()) th.join();
  }
};

struct PermStream {
  hipStream_t s = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~PermStream() {
    if (s) (void)hipStreamDestroy(s);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

}  // namespace

extern "C" {

int lsspa_debug_perm_indices(uint64_t seed, uint64_t r, int32_t side, int64_t n, uint32_t* out) try {
  if (!out || n < 1 || n >= (1ll << 31) || side < 0 || side > 1) return LSSPA_ERR_ARG;
  perm_indices(seed, r, side, n, out);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_NOMEM;
}

int lsspa_debug_perm_plan(int64_t R, int64_t N, int64_t M, int32_t p, int64_t block, int64_t* plan10) try {
  if (!plan10) return LSSPA_ERR_ARG;
  PermPlan P;
  if (perm_plan(R, N, M, p, block, P)) return LSSPA_ERR_ARG;
  const int64_t v[10] = {P.block, P.n_blocks, P.rps[0], P.rps[1], P.slices[0], P.slices[1], P.cb, P.ldi[0], P.ldi[1],
                         P.rep_bytes};
  std::copy(v, v + 10, plan10);
  return LSSPA_OK;
} catch (...) {
  return LSSPA_ERR_NOMEM;
}

int lsspa_perm_load(lsspa_ctx* ctx, const void* X_train, int64_t ld_train, const void* y_train, int64_t N,
                    const void* X_test, int64_t ld_test, const void* y_test, int64_t M, int32_t p, double reg,
                    int32_t dtype, int32_t location) try {
  if (!ctx) return LSSPA_ERR_ARG;
  char msg[240];
  if (p < 1 || p > GROUPS_MAX_P) {
    snprintf(msg, sizeof msg, "lsspa_perm_load takes 1 <= p <= %d columns, of which the enumeration without labels takes "
             "p <= %d (%d given)", GROUPS_MAX_P, MULTI_MAX_P, (int)p);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  PermPlan P;
  if (const char* why = perm_plan(1, N, M, p, 0, P)) {
    snprintf(msg, sizeof msg, "lsspa_perm_load: %s", why);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  if (!multi_sides_ok(X_train, ld_train, y_train, 1, N, X_test, ld_test, y_test, 1, M, p, 1, reg, dtype, location))
    return ctx->fail(LSSPA_ERR_ARG, "lsspa_perm_load: NULL array, N or M < 1, ld < p, reg not finite and >= 0, or bad "
                                    "dtype / location");
  HIPCHK(hipSetDevice(ctx->device));
  PermWork& W = ctx->perm;
  W.loaded = false;
  W.mw.loaded = false;
  std::vector<double> G, g, H, h, yy;
  double gram_ms = 0.0;
  TRY(multi_reduce_sides(ctx, X_train, ld_train, y_train, 1, N, X_test, ld_test, y_test, 1, M, p, 1, reg, dtype, location,
                         G, g, H, h, yy, gram_ms));
  TRY(reduced_check_yy(ctx, 1, yy.data(), "y_test is identically zero (or NaN)"));
  const void* X[2] = {X_train, X_test};
  const void* y[2] = {y_train, y_test};
  const int64_t n[2] = {N, M}, ld[2] = {ld_train, ld_test};
  for (int s = 0; s < 2; ++s) {
    TRY(dev_alloc(ctx, W.X(s), (size_t)n[s] * P.ldx));
    TRY(dev_alloc(ctx, W.y(s), (size_t)n[s]));
    TRY(load_rows(ctx, W.stage_x, W.stage_y, X[s], ld[s], y[s], n[s], p, dtype, location,
                  [&](const void* sx, const void* sy, int64_t nr, int64_t r0) {
                    return launch_perm_pack(sx, ld[s], sy, nr, p, dtype == LSSPA_F32, W.X(s).ptr, P.ldx, W.y(s).ptr, r0,
                                            ctx->stream);
                  }));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  dev_free(W.stage_x);
  dev_free(W.stage_y);
  // the observed g, h beside the form's own, which are the response slots of a block of replicates (perm_slots)
  TRY(reduced_store(ctx, W.mw.rf, p, 1, G.data(), g.data(), H.data(), h.data(), yy.data(), W.obs_g, W.obs_h));
  W.p = p;
  W.mw.rf.m = 0;
  W.mw.gram_ms = gram_ms;
  W.n[0] = N;
  W.n[1] = M;
  for (double& v : W.ms) v = 0.0;
  W.mw.loaded = true;
  W.loaded = true;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_perm_observed(lsspa_ctx* ctx, const int32_t* labels, int32_t g, double* phi, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(perm_need_loaded(ctx));
  if (!phi) return ctx->fail(LSSPA_ERR_ARG, "lsspa_perm_observed: phi is NULL");
  TRY(perm_players(ctx, "lsspa_perm_observed", labels, g));
  HIPCHK(hipSetDevice(ctx->device));
  PermWork& W = ctx->perm;
  TRY(perm_slots(ctx, 1));
  HIPCHK(launch_perm_fill(W.obs_g.ptr, W.p, 1, W.mw.rf.g.ptr, ctx->stream));
  HIPCHK(launch_perm_fill(W.obs_h.ptr, W.p, 1, W.mw.rf.h.ptr, ctx->stream));
  int32_t bits = 0;
  TRY(perm_enumerate(ctx, labels, g, 1, phi, &bits));
  if (info) *info = bits;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_perm_run(lsspa_ctx* ctx, const int32_t* labels, int32_t g, int64_t R, uint64_t seed, int64_t first,
                   int32_t sides, int64_t block, double* phi, double* gperm, double* hperm, int32_t* info) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(perm_need_loaded(ctx));
  if (!phi || first < 0 || sides < 1 || sides > 3)
    return ctx->fail(LSSPA_ERR_ARG, "lsspa_perm_run: phi is NULL, first < 0, or sides is not 1 (train), 2 (test) or 3 (both)");
  TRY(perm_players(ctx, "lsspa_perm_run", labels, g));
  PermWork& W = ctx->perm;
  const int p = W.p, d = labels ? g : p;
  PermPlan P;
  if (const char* why = perm_plan(R, W.n[0], W.n[1], p, block, P)) {
    char msg[200];
    snprintf(msg, sizeof msg, "lsspa_perm_run: %s", why);
    return ctx->fail(LSSPA_ERR_ARG, msg);
  }
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t blk = P.block, sets = (blk + 15) / 16;
  TRY(perm_slots(ctx, blk));
  for (int s = 0; s < 2; ++s) {
    if (!((sides >> s) & 1)) continue;
    TRY(dev_alloc(ctx, W.part(s), (size_t)P.slices[s] * sets * P.cb * 256));
    for (int b = 0; b < 2; ++b) {
      const size_t cnt = (size_t)blk * P.ldi[s];
      TRY(dev_alloc(ctx, W.idx[b][s], cnt));
      if (W.pin_count[b][s] < cnt) {
        if (W.pin[b][s]) (void)hipHostFree(W.pin[b][s]);
        W.pin[b][s] = nullptr;
        W.pin_count[b][s] = 0;
        if (hipHostMalloc((void**)&W.pin[b][s], cnt * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) {
          W.pin[b][s] = nullptr;
          return ctx->fail(LSSPA_ERR_NOMEM, "pinned host memory for the index rows of a block of replicates");
        }
        W.pin_count[b][s] = cnt;
      }
    }
  }
  // the side that is not permuted keeps its observed g or h in every slot
  if (!(sides & 1)) HIPCHK(launch_perm_fill(W.obs_g.ptr, p, (int)blk, W.mw.rf.g.ptr, ctx->stream));
  if (!(sides & 2)) HIPCHK(launch_perm_fill(W.obs_h.ptr, p, (int)blk, W.mw.rf.h.ptr, ctx->stream));
  PermStream up;
  HIPCHK(hipStreamCreateWithFlags(&up.s, hipStreamNonBlocking));
  for (hipEvent_t& e : up.ev) HIPCHK(hipEventCreate(&e));
  for (double& v : W.ms) v = 0.0;
  const int device = ctx->device;
  PermProducer prod[2];
  auto produce = [&](int64_t b) {
    PermProducer& J = prod[b & 1];
    const int64_t nb = std::min(blk, R - b * blk);
    const uint64_t r0 = (uint64_t)first + (uint64_t)(b * blk);
    J.err = hipSuccess;
    J.draw_ms = J.upload_ms = 0.0;
    J.th = std::thread([&W, &P, &J, &up, b, nb, r0, seed, sides, device] {
      using clk = std::chrono::steady_clock;
      J.err = hipSetDevice(device);
      for (int s = 0; s < 2 && J.err == hipSuccess; ++s) {
        if (!((sides >> s) & 1)) continue;
        const auto t0 = clk::now();
        perm_draw_block(seed, r0, (int)nb, s, W.n[s], P.ldi[s], W.pin[b & 1][s], 16);
        const auto t1 = clk::now();
        J.err = hipMemcpyAsync(W.idx[b & 1][s].ptr, W.pin[b & 1][s], sizeof(uint32_t) * (size_t)nb * P.ldi[s],
                               hipMemcpyHostToDevice, up.s);
        if (J.err == hipSuccess) J.err = hipStreamSynchronize(up.s);
        const auto t2 = clk::now();
        J.draw_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
        J.upload_ms += std::chrono::duration<double, std::milli>(t2 - t1).count();
      }
    });
  };
  int32_t all_bits = 0;
  produce(0);
  for (int64_t b = 0; b < P.n_blocks; ++b) {
    const int64_t nb = std::min(blk, R - b * blk);
    PermProducer& J = prod[b & 1];
    J.wait();
    if (J.err != hipSuccess) return ctx->fail(LSSPA_ERR_HIP, "upload of a block's index rows", J.err);
    W.ms[0] += J.draw_ms;
    W.ms[1] += J.upload_ms;
    // block b + 1 is drawn and uploaded while the GPU works on block b: its buffers were last read by block b - 1,
    // whose enumeration this thread has waited for
    if (b + 1 < P.n_blocks) produce(b + 1);
    HIPCHK(hipEventRecord(up.ev[0], ctx->stream));
    for (int s = 0; s < 2; ++s) {
      if (!((sides >> s) & 1)) continue;
      HIPCHK(launch_perm_xty(P, s, W.X(s).ptr, W.y(s).ptr, W.idx[b & 1][s].ptr, W.n[s], (int)nb, W.part(s).ptr,
                             ctx->stream));
      HIPCHK(launch_perm_reduce(P, s, W.part(s).ptr, p, (int)nb, s == 0 ? 1.0 / (double)W.n[0] : 1.0,
                                s == 0 ? W.mw.rf.g.ptr : W.mw.rf.h.ptr, ctx->stream));
    }
    HIPCHK(hipEventRecord(up.ev[1], ctx->stream));
    const size_t at = (size_t)(b * blk) * p;
    if (gperm)
      HIPCHK(hipMemcpyAsync(gperm + at, W.mw.rf.g.ptr, sizeof(double) * (size_t)nb * p, hipMemcpyDeviceToHost, ctx->stream));
    if (hperm)
      HIPCHK(hipMemcpyAsync(hperm + at, W.mw.rf.h.ptr, sizeof(double) * (size_t)nb * p, hipMemcpyDeviceToHost, ctx->stream));
    int32_t bits = 0;
    TRY(perm_enumerate(ctx, labels, g, nb, phi + (size_t)(b * blk) * d, &bits));
    all_bits |= bits;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, up.ev[0], up.ev[1]));
    W.ms[2] += ms;
    W.ms[3] += W.mw.enum_ms;
  }
  if (info) *info = all_bits;
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_perm_get_gram(lsspa_ctx* ctx, double* G, double* g, double* H, double* h, double* yy) try {
  if (!ctx) return LSSPA_ERR_ARG;
  TRY(perm_need_loaded(ctx));
  reduced_get(ctx->perm.mw.rf, G, g, H, h, yy);
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

int lsspa_perm_timing(const lsspa_ctx* ctx, double* draw_ms, double* upload_ms, double* xty_ms, double* enum_ms) try {
  if (!ctx) return LSSPA_ERR_ARG;
  if (draw_ms) *draw_ms = ctx->perm.ms[0];
  if (upload_ms) *upload_ms = ctx->perm.ms[1];
  if (xty_ms) *xty_ms = ctx->perm.ms[2];
  if (enum_ms) *enum_ms = ctx->perm.ms[3];
  return LSSPA_OK;
} catch (...) {
  return abi_caught(const_cast<lsspa_ctx*>(ctx));
}

int lsspa_perm_free(lsspa_ctx* ctx) try {
  if (!ctx) return LSSPA_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->perm.release();
  return LSSPA_OK;
} catch (...) {
  return abi_caught(ctx);
}

}  // extern "C"
