// K-fold cross-validation (lsspa_cv_load .. lsspa_cv_free; DESIGN.md, "K-fold cross-validation"): the small kernels
// between the bootstrap's weighted Gram pass (k_boot.hip) and the enumerations of k_subsets.hip and, over groups of
// columns (lsspa_cv_groups_*, p <= 64), of k_groups.hip.  fp64 throughout.
//
// The rows z_i = [x_i, y_i] are packed once (launch_boot_pack).  Fold f's Gram S_f = sum_{i in f} z_i z_i^T is the
// bootstrap's weighted Gram with the indicator of the fold as the weights: cv_weights_kernel writes those from the
// fold labels on the device, launch_boot_gram / launch_boot_reduce do the rest.  cv_finalize_kernel then forms the
// fold problems in the replicate layout the enumerations read: fold f is tested on its own rows and trained on the
// others',
//   G_f = (sum_{j != f} S_j)[:p,:p] / (N - n_f) + reg I,   g_f likewise,   H_f = S_f[:p,:p],   h_f = S_f[:p,p],
// the sums over j ascending (added, not subtracted from a total: no cancellation), and every fold divides by the same
// pooled ||y||^2 = sum_j S_j[p][p], so that the folds' values add up to the cross-validated R^2.
#include "kernels.h"

namespace lsspa {
namespace {

__global__ __launch_bounds__(256) void cv_weights_kernel(const int32_t* __restrict__ fid, int64_t n,
                                                         double* __restrict__ wt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) wt[(int64_t)blockIdx.y * n + i] = fid[i] == (int32_t)blockIdx.y ? 1.0 : 0.0;
}

__global__ __launch_bounds__(256) void cv_finalize_kernel(const double* __restrict__ S, const int32_t* __restrict__ nf,
                                                          int64_t n, int p, int folds, double reg,
                                                          double* __restrict__ G, double* __restrict__ g,
                                                          double* __restrict__ H, double* __restrict__ h,
                                                          double* __restrict__ inv_yy) {
  const int f = blockIdx.x, c = p + 1;
  const int64_t cc = (int64_t)c * c;
  const double W = (double)(n - nf[f]);
  const double* T = S + f * cc;
  for (int e = threadIdx.x; e < p * p; e += 256) {
    const int i = e / p, j = e - i * p;
    double s = 0.0;
    for (int k = 0; k < folds; ++k)
      if (k != f) s += S[k * cc + i * c + j];
    G[(int64_t)f * p * p + e] = s / W + (i == j ? reg : 0.0);
    H[(int64_t)f * p * p + e] = T[i * c + j];
  }
  if ((int)threadIdx.x < p) {
    const int i = threadIdx.x;
    double s = 0.0;
    for (int k = 0; k < folds; ++k)
      if (k != f) s += S[k * cc + i * c + p];
    g[(int64_t)f * p + i] = s / W;
    h[(int64_t)f * p + i] = T[i * c + p];
  }
  if (threadIdx.x == 0) {
    double yy = 0.0;
    for (int k = 0; k < folds; ++k) yy += S[k * cc + p * c + p];
    inv_yy[f] = 1.0 / yy;
  }
}

__global__ __launch_bounds__(64) void cv_foldsum_kernel(const double* __restrict__ out, int p, int folds,
                                                        double* __restrict__ phi_fold, double* __restrict__ phi) {
  const int j = threadIdx.x;
  if (j >= p) return;
  double s = 0.0;
  for (int f = 0; f < folds; ++f) {
    const double v = out[f * (p + 1) + j] - out[f * (p + 1) + p];
    phi_fold[f * p + j] = v;
    s = f == 0 ? v : s + v;
  }
  phi[j] = s;
}

// cv_foldsum_kernel over groups: the enumeration's columns are in the layout's numbering, gid[r] the caller's label of
// the layout's group r (GroupLayout::gid, by value)
struct CvGroupIds {
  uint8_t id[GROUPS_MAX_G];
};

__global__ __launch_bounds__(64) void cv_groups_foldsum_kernel(const double* __restrict__ out, int ng, int folds,
                                                               CvGroupIds ids, double* __restrict__ phi_fold,
                                                               double* __restrict__ phi) {
  const int r = threadIdx.x;
  if (r >= ng) return;
  const int k = ids.id[r];
  double s = 0.0;
  for (int f = 0; f < folds; ++f) {
    const double v = out[f * (ng + 1) + r] - out[f * (ng + 1) + ng];
    phi_fold[f * ng + k] = v;
    s = f == 0 ? v : s + v;
  }
  phi[k] = s;
}

}  // namespace

hipError_t launch_cv_weights(const int32_t* fid, int64_t n, int folds, double* wt, hipStream_t st) {
  if (!fid || !wt || n < 1 || n >= (1ll << 31) || folds < 2 || folds > CV_MAX_FOLDS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cv_weights_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)folds), dim3(256), 0, st, fid, n,
                     wt);
  return hipGetLastError();
}

hipError_t launch_cv_finalize(const double* S, const int32_t* nf, int64_t n, int p, int folds, double reg, double* G,
                              double* g, double* H, double* h, double* inv_yy, hipStream_t st) {
  // p up to GROUPS_MAX_P: the grouped load (lsspa_cv_groups_load); the kernel strides over p^2 and has 256 >= p threads
  if (!S || !nf || !G || !g || !H || !h || !inv_yy || n < 2 || p < 1 || p > GROUPS_MAX_P || folds < 2 ||
      folds > CV_MAX_FOLDS)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(cv_finalize_kernel, dim3((unsigned)folds), dim3(256), 0, st, S, nf, n, p, folds, reg, G, g, H, h,
                     inv_yy);
  return hipGetLastError();
}

hipError_t launch_cv_foldsum(const double* out, int p, int folds, double* phi_fold, double* phi, hipStream_t st) {
  if (!out || !phi_fold || !phi || p < 1 || p > SUBSETS_MAX_P || folds < 2 || folds > CV_MAX_FOLDS)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(cv_foldsum_kernel, dim3(1), dim3(64), 0, st, out, p, folds, phi_fold, phi);
  return hipGetLastError();
}

hipError_t launch_cv_groups_foldsum(const double* out, int ng, int folds, const int* gid, double* phi_fold, double* phi,
                                    hipStream_t st) {
  if (!out || !gid || !phi_fold || !phi || ng < 1 || ng > GROUPS_MAX_G || folds < 2 || folds > CV_MAX_FOLDS)
    return hipErrorInvalidValue;
  CvGroupIds ids{};
  uint32_t seen = 0u;
  for (int r = 0; r < ng; ++r) {                     // a permutation of 0 .. ng-1: every entry of phi is written once
    if (gid[r] < 0 || gid[r] >= ng || ((seen >> gid[r]) & 1u)) return hipErrorInvalidValue;
    seen |= 1u << gid[r];
    ids.id[r] = (uint8_t)gid[r];
  }
  hipLaunchKernelGGL(cv_groups_foldsum_kernel, dim3(1), dim3(64), 0, st, out, ng, folds, ids, phi_fold, phi);
  return hipGetLastError();
}

// ---- the ridge path (lsspa_cv_path_shapley, lsspa_cv_path_groups_shapley; DESIGN.md, "Ridge path of the K-fold CV") ----
// A block of nl ridge values on the loaded per-fold Grams: problem (l, f) sits at replicate l folds + f of the layout
// above, so that the enumerations run the nl folds problems as replicates of shared grids.  The kernels are the three
// above with the ridge value as a second grid dimension: the same expressions in the same order, so that problem (l, f)
// has the bits cv_finalize_kernel writes for fold f with reg = regs[l], and row l of the sums the bits of
// cv_foldsum_kernel / cv_groups_foldsum_kernel on those folds.  The replicate layout is dense (one stride for G, g, H,
// h and inv_yy: kernels.h, SubsetArgs), so H_f, h_f and 1 / ||y||^2, which do not depend on the ridge value, are
// written once per problem, not once per fold.
namespace {

__global__ __launch_bounds__(256) void cv_path_finalize_kernel(const double* __restrict__ S,
                                                               const int32_t* __restrict__ nf,
                                                               const double* __restrict__ regs, int64_t n, int p,
                                                               int folds, double* __restrict__ G,
                                                               double* __restrict__ g, double* __restrict__ H,
                                                               double* __restrict__ h, double* __restrict__ inv_yy) {
  const int f = blockIdx.x, c = p + 1;
  const int64_t r = (int64_t)blockIdx.y * folds + f;      // the problem's replicate
  const int64_t cc = (int64_t)c * c;
  const double reg = regs[blockIdx.y];
  const double W = (double)(n - nf[f]);
  const double* T = S + f * cc;
  for (int e = threadIdx.x; e < p * p; e += 256) {
    const int i = e / p, j = e - i * p;
    double s = 0.0;
    for (int k = 0; k < folds; ++k)
      if (k != f) s += S[k * cc + i * c + j];
    G[r * p * p + e] = s / W + (i == j ? reg : 0.0);
    H[r * p * p + e] = T[i * c + j];
  }
  if ((int)threadIdx.x < p) {
    const int i = threadIdx.x;
    double s = 0.0;
    for (int k = 0; k < folds; ++k)
      if (k != f) s += S[k * cc + i * c + p];
    g[r * p + i] = s / W;
    h[r * p + i] = T[i * c + p];
  }
  if (threadIdx.x == 0) {
    double yy = 0.0;
    for (int k = 0; k < folds; ++k) yy += S[k * cc + p * c + p];
    inv_yy[r] = 1.0 / yy;
  }
}

__global__ __launch_bounds__(64) void cv_path_foldsum_kernel(const double* __restrict__ out, int p, int folds,
                                                             double* __restrict__ phi_fold, double* __restrict__ phi) {
  const int j = threadIdx.x;
  if (j >= p) return;
  const int64_t l = blockIdx.x;
  out += l * folds * (p + 1);
  phi_fold += l * folds * p;
  double s = 0.0;
  for (int f = 0; f < folds; ++f) {
    const double v = out[f * (p + 1) + j] - out[f * (p + 1) + p];
    phi_fold[f * p + j] = v;
    s = f == 0 ? v : s + v;
  }
  phi[l * p + j] = s;
}

__global__ __launch_bounds__(64) void cv_path_groups_foldsum_kernel(const double* __restrict__ out, int ng, int folds,
                                                                    CvGroupIds ids, double* __restrict__ phi_fold,
                                                                    double* __restrict__ phi) {
  const int r = threadIdx.x;
  if (r >= ng) return;
  const int64_t l = blockIdx.x;
  out += l * folds * (ng + 1);
  phi_fold += l * folds * ng;
  const int k = ids.id[r];
  double s = 0.0;
  for (int f = 0; f < folds; ++f) {
    const double v = out[f * (ng + 1) + r] - out[f * (ng + 1) + ng];
    phi_fold[f * ng + k] = v;
    s = f == 0 ? v : s + v;
  }
  phi[l * ng + k] = s;
}

}  // namespace

hipError_t launch_cv_path_finalize(const double* S, const int32_t* nf, const double* regs, int nl, int64_t n, int p,
                                   int folds, double* G, double* g, double* H, double* h, double* inv_yy,
                                   hipStream_t st) {
  if (!S || !nf || !regs || !G || !g || !H || !h || !inv_yy || nl < 1 || nl > CV_PATH_MAX_REGS || n < 2 || p < 1 ||
      p > GROUPS_MAX_P || folds < 2 || folds > CV_MAX_FOLDS)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(cv_path_finalize_kernel, dim3((unsigned)folds, (unsigned)nl), dim3(256), 0, st, S, nf, regs, n, p,
                     folds, G, g, H, h, inv_yy);
  return hipGetLastError();
}

hipError_t launch_cv_path_foldsum(const double* out, int p, int folds, int nl, double* phi_fold, double* phi,
                                  hipStream_t st) {
  if (!out || !phi_fold || !phi || p < 1 || p > SUBSETS_MAX_P || folds < 2 || folds > CV_MAX_FOLDS || nl < 1 ||
      nl > CV_PATH_MAX_REGS)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(cv_path_foldsum_kernel, dim3((unsigned)nl), dim3(64), 0, st, out, p, folds, phi_fold, phi);
  return hipGetLastError();
}

hipError_t launch_cv_path_groups_foldsum(const double* out, int ng, int folds, int nl, const int* gid, double* phi_fold,
                                         double* phi, hipStream_t st) {
  if (!out || !gid || !phi_fold || !phi || ng < 1 || ng > GROUPS_MAX_G || folds < 2 || folds > CV_MAX_FOLDS || nl < 1 ||
      nl > CV_PATH_MAX_REGS)
    return hipErrorInvalidValue;
  CvGroupIds ids{};
  uint32_t seen = 0u;
  for (int r = 0; r < ng; ++r) {                     // a permutation of 0 .. ng-1: every entry of phi is written once
    if (gid[r] < 0 || gid[r] >= ng || ((seen >> gid[r]) & 1u)) return hipErrorInvalidValue;
    seen |= 1u << gid[r];
    ids.id[r] = (uint8_t)gid[r];
  }
  hipLaunchKernelGGL(cv_path_groups_foldsum_kernel, dim3((unsigned)nl), dim3(64), 0, st, out, ng, folds, ids, phi_fold,
                     phi);
  return hipGetLastError();
}

// ---- the sampled attribution (lsspa_cv_lift_*; DESIGN.md, "Sampled K-fold CV attribution") -----------------------------
// p <= 127: the rows are packed SORTED BY FOLD (stable in row order), so that fold f is a contiguous slice and its Gram
// S_f one launch_gram of any width on the slice.  cv_lift_finalize_kernel is cv_finalize_kernel on those Grams -- the
// same expressions in the same order, S_f read from launch_gram's [128][128] buffers -- and writes the fold problems at
// the one stride the fold launch of k_small.hip reads (rows of CV_LIFT_LD doubles), with the augmented rows' diagonals
// the one-response path gives a problem (2 ||y_train||^2 / N_train + 1, 2 ||y_test||^2 + 1).  cv_lift_fold_kernel takes
// that launch's raw lifts [ordering][fold][p] to a batch of samples [sample][folds + 1][d]: the folds' rows, then their
// sum in ascending fold order.
namespace {

template <typename T>
__global__ __launch_bounds__(256) void cv_lift_pack_kernel(const T* __restrict__ X, int64_t ld, const T* __restrict__ y,
                                                           int64_t rows, int p, const int32_t* __restrict__ dest,
                                                           double* __restrict__ Xs, double* __restrict__ ys) {
  // 128 threads a row, two rows a workgroup
  const int64_t i = (int64_t)blockIdx.x * 2 + (threadIdx.x >> 7);
  const int c = threadIdx.x & 127;
  if (i >= rows) return;
  const int64_t r = dest[i];
  Xs[r * CV_LIFT_LD + c] = c < p ? (double)X[i * ld + c] : 0.0;
  if (c == 0) ys[r] = (double)y[i];
}

__global__ __launch_bounds__(256) void cv_lift_finalize_kernel(const double* __restrict__ S,
                                                               const int32_t* __restrict__ nf, int64_t n, int p,
                                                               int folds, double reg, double* __restrict__ G,
                                                               double* __restrict__ g, double* __restrict__ H,
                                                               double* __restrict__ h, double* __restrict__ inv_yy,
                                                               double* __restrict__ aug) {
  constexpr int c = CV_LIFT_LD;                        // row length of S_f and of the problems
  constexpr int64_t cc = (int64_t)c * c;
  const int f = blockIdx.x;
  const double W = (double)(n - nf[f]);
  const double* T = S + f * cc;
  for (int e = threadIdx.x; e < p * p; e += 256) {
    const int i = e / p, j = e - i * p;
    const int lo = (i >= j ? i : j) * c + (i >= j ? j : i);      // launch_gram's buffer is valid in its lower part
    double s = 0.0;
    for (int k = 0; k < folds; ++k)
      if (k != f) s += S[k * cc + lo];
    G[f * cc + i * c + j] = s / W + (i == j ? reg : 0.0);
    H[f * cc + i * c + j] = T[lo];
  }
  if ((int)threadIdx.x < p) {
    const int i = threadIdx.x;
    double s = 0.0;
    for (int k = 0; k < folds; ++k)
      if (k != f) s += S[k * cc + p * c + i];      // (row p, as launch_gram_finalize reads launch_gram's buffer)
    g[f * c + i] = s / W;
    h[f * c + i] = T[p * c + i];
  }
  if (threadIdx.x == 0) {
    double yy = 0.0, yt = 0.0;
    for (int k = 0; k < folds; ++k) yy += S[k * cc + p * c + p];
    for (int k = 0; k < folds; ++k)
      if (k != f) yt += S[k * cc + p * c + p];
    inv_yy[f] = 1.0 / yy;
    aug[2 * f] = 2.0 * (yt / W) + 1.0;
    aug[2 * f + 1] = 2.0 * T[p * c + p] + 1.0;
  }
}

// One thread per (sample, player k): the folds' entries one after the other, their running sum behind them.  A fold's
// entry of one ordering is its lift (no map) or the sum of the group's columns in ascending column order from 0.0
// (k_players.hip's order); a pair's is 0.5 a + 0.5 b of its two orderings' entries.
__global__ __launch_bounds__(256) void cv_lift_fold_kernel(const double* __restrict__ raw, int p, int folds, int per,
                                                           const int32_t* __restrict__ off,
                                                           const int32_t* __restrict__ cols, int d, int64_t n_samples,
                                                           double* __restrict__ batch) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= n_samples * d) return;
  const int64_t s = o / d;
  const int k = (int)(o - s * d);
  const int c0 = off ? off[k] : 0, c1 = off ? off[k + 1] : 0;
  double* const dst = batch + s * (folds + 1) * d + k;
  double sum = 0.0;
  for (int f = 0; f < folds; ++f) {
    double e[2] = {0.0, 0.0};
    for (int r = 0; r < per; ++r) {
      const double* row = raw + ((s * per + r) * folds + f) * p;
      if (off) {
        double a = 0.0;
        for (int c = c0; c < c1; ++c) a += row[cols[c]];
        e[r] = a;
      } else {
        e[r] = row[k];
      }
    }
    const double v = per == 2 ? 0.5 * e[0] + 0.5 * e[1] : e[0];
    dst[(int64_t)f * d] = v;
    sum = f == 0 ? v : sum + v;
  }
  dst[(int64_t)folds * d] = sum;
}

}  // namespace

hipError_t launch_cv_lift_pack(const void* X, int64_t ld, const void* y, int64_t rows, int p, int is_f32,
                               const int32_t* dest, double* Xs, double* ys, hipStream_t st) {
  if (!X || !y || !dest || !Xs || !ys || rows < 1 || rows >= (1ll << 31) || p < 1 || p >= CV_LIFT_LD || ld < p)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((rows + 1) / 2));
  if (is_f32)
    hipLaunchKernelGGL(cv_lift_pack_kernel<float>, grid, dim3(256), 0, st, (const float*)X, ld, (const float*)y, rows, p,
                       dest, Xs, ys);
  else
    hipLaunchKernelGGL(cv_lift_pack_kernel<double>, grid, dim3(256), 0, st, (const double*)X, ld, (const double*)y, rows,
                       p, dest, Xs, ys);
  return hipGetLastError();
}

hipError_t launch_cv_lift_finalize(const double* S, const int32_t* nf, int64_t n, int p, int folds, double reg, double* G,
                                   double* g, double* H, double* h, double* inv_yy, double* aug, hipStream_t st) {
  if (!S || !nf || !G || !g || !H || !h || !inv_yy || !aug || n < 2 || p < 1 || p >= CV_LIFT_LD || folds < 2 ||
      folds > CV_MAX_FOLDS)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(cv_lift_finalize_kernel, dim3((unsigned)folds), dim3(256), 0, st, S, nf, n, p, folds, reg, G, g, H,
                     h, inv_yy, aug);
  return hipGetLastError();
}

hipError_t launch_cv_lift_fold(const double* raw, int p, int folds, int per, const int32_t* off, const int32_t* cols,
                               int d, int64_t n_samples, double* batch, hipStream_t st) {
  // (off and cols are the library's own tables: player_map_build has checked that every column index is in 0 .. p-1)
  if (!raw || !batch || p < 1 || p >= CV_LIFT_LD || folds < 2 || folds > CV_MAX_FOLDS || (per != 1 && per != 2) ||
      d < 1 || d > p || (off ? !cols : d != p) || n_samples < 1 || n_samples * d >= (1ll << 31) * 256)
    return hipErrorInvalidValue;
  const int64_t total = n_samples * d;
  hipLaunchKernelGGL(cv_lift_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, raw, p, folds, per,
                     off, cols, d, n_samples, batch);
  return hipGetLastError();
}

}  // namespace lsspa
