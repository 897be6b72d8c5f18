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

}  // namespace lsspa
