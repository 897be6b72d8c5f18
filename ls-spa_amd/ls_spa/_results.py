"""Result container and input validation of the LS-SPA surface.

Mirrors cvxgrp/ls-spa ``ls_spa/ls_spa.py``: ``ShapleyResults`` (:34-70, same field
order, same dashboard text), ``SizeIncompatible`` (:73-78) and ``validate_data``
(:81-100, same four checks in the same order, same messages).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


def _head(values, limit=5):
    flat = np.asarray(values).ravel()
    shown = ", ".join(f"{v:.2f}" for v in flat[:limit])
    return f"({shown}, ...)" if flat.size > limit else f"({shown})"


@dataclass
class ShapleyResults:
    attribution: np.ndarray
    theta: np.ndarray
    overall_error: float
    attribution_errors: np.ndarray
    r_squared: float
    error_history: np.ndarray | None
    attribution_history: np.ndarray | None

    def __repr__(self):
        pad = " " * 8
        lines = [
            "",
            f"{pad}p = {np.asarray(self.attribution).size}",
            f"{pad}Out-of-sample R^2 with all features: {self.r_squared:.2f}",
            "",
            f"{pad}Shapley attribution: {_head(self.attribution)}",
            f"{pad}Estimated error in Shapley attribution: {self.overall_error:.2E}",
            "",
            f"{pad}Fitted coeficients with all features: {_head(self.theta)}",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class InteractionResults:
    """What ``ls_spa_interactions`` returns.  ``interactions`` [p][p] is the Shapley interaction matrix in SHAP's
    convention: symmetric, half the pairwise interaction index off the diagonal, row i summing to ``attribution[i]``
    and the whole matrix to ``r_squared``.  The other three fields are those of ``ls_spa(method='subsets')``.  With
    ``groups=`` the players are the g groups of columns: ``interactions`` is [g][g], ``attribution`` [g], the whole matrix
    sums to ``r_squared`` minus the R^2 of the baseline columns alone, and ``theta`` keeps length p."""
    interactions: np.ndarray
    attribution: np.ndarray
    theta: np.ndarray
    r_squared: float

    def __repr__(self):
        pad = " " * 8
        inter = np.asarray(self.interactions)
        off = inter - np.diag(np.diag(inter))
        lines = [
            "",
            f"{pad}p = {np.asarray(self.attribution).size}",
            f"{pad}Out-of-sample R^2 with all features: {self.r_squared:.2f}",
            "",
            f"{pad}Shapley attribution: {_head(self.attribution)}",
            f"{pad}Main effects (diagonal): {_head(np.diag(inter))}",
            f"{pad}Largest pairwise interaction: {float(np.abs(off).max()) if off.size else 0.0:.2E}",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class SampledInteractionResults:
    """What ``ls_spa_interactions_sampled`` returns.  ``interactions`` [d][d] is the estimated Shapley interaction matrix
    in SHAP's convention (half the estimated pairwise index off the diagonal, row a summing to ``attribution[a]``, the
    whole matrix to ``r_squared`` -- minus the R^2 of the baseline with ``groups=``); ``interaction_errors`` [d][d] the
    standard errors of its off-diagonal entries (0 on the diagonal, ``inf`` for a pair no sample hit) and ``counts``
    [d][d] the number of samples in which the pair was adjacent; ``n_samples`` the samples drawn (three orderings each).
    ``attribution`` is the mean of all 3 n lift vectors; ``theta`` and ``r_squared`` are those of the full fit."""
    interactions: np.ndarray
    attribution: np.ndarray
    theta: np.ndarray
    r_squared: float
    interaction_errors: np.ndarray
    counts: np.ndarray
    n_samples: int

    def __repr__(self):
        pad = " " * 8
        inter = np.asarray(self.interactions)
        off = inter - np.diag(np.diag(inter))
        err = np.asarray(self.interaction_errors)
        finite = err[np.isfinite(err)]
        lines = [
            "",
            f"{pad}d = {np.asarray(self.attribution).size}, {self.n_samples} samples",
            f"{pad}Out-of-sample R^2 with all features: {self.r_squared:.2f}",
            "",
            f"{pad}Shapley attribution: {_head(self.attribution)}",
            f"{pad}Largest pairwise interaction: {float(np.abs(off).max()) if off.size else 0.0:.2E}",
            f"{pad}Largest standard error: {float(finite.max()) if finite.size else float('nan'):.2E}"
            f" ({int((np.asarray(self.counts) == 0).sum() - len(inter)) // 2} pairs never hit)",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class MultiResponseResults:
    """What ``ls_spa_multi`` returns for m responses on one design matrix.  ``attribution`` [m][p]: row r is the exact
    Shapley attribution of response r, what ``ls_spa(method='subsets')`` returns for that column alone; ``theta`` [m][p]
    the full-model coefficients of each response; ``r_squared`` [m] their out-of-sample R^2 -- row r of ``attribution``
    sums to ``r_squared[r]``."""
    attribution: np.ndarray
    theta: np.ndarray
    r_squared: np.ndarray

    def __repr__(self):
        pad = " " * 8
        att = np.asarray(self.attribution)
        lines = [
            "",
            f"{pad}p = {att.shape[1]}, m = {att.shape[0]} responses",
            f"{pad}Out-of-sample R^2 with all features: {_head(self.r_squared)}",
            "",
            f"{pad}Shapley attribution of response 0: {_head(att[0])}",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class MultiGroupResults:
    """What ``ls_spa_multi(groups=)`` returns for m responses on one design matrix whose columns form g groups.
    ``attribution`` [m][g]: row r is the exact Shapley attribution of response r over the groups, what
    ``ls_spa(method='subsets', groups=)`` returns for that column alone; ``theta`` [m][p] the full-model coefficients of
    each response; ``r_squared`` [m] their out-of-sample R^2 and ``baseline_r_squared`` [m] that of the baseline columns
    alone (0 without a baseline) -- row r of ``attribution`` sums to ``r_squared[r] - baseline_r_squared[r]``."""
    attribution: np.ndarray
    theta: np.ndarray
    r_squared: np.ndarray
    baseline_r_squared: np.ndarray

    def __repr__(self):
        pad = " " * 8
        att = np.asarray(self.attribution)
        lines = [
            "",
            f"{pad}g = {att.shape[1]} groups, p = {np.asarray(self.theta).shape[1]}, m = {att.shape[0]} responses",
            f"{pad}Out-of-sample R^2 with all columns: {_head(self.r_squared)}",
            f"{pad}Out-of-sample R^2 of the baseline: {_head(self.baseline_r_squared)}",
            "",
            f"{pad}Shapley attribution of response 0: {_head(att[0])}",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class OwenResults:
    """What ``ls_spa_owen`` returns for p columns in g groups.  ``attribution`` [p]: the exact Owen value of every
    column, 0.0 on baseline columns; ``group_attribution`` [g]: the groups' Shapley values, what
    ``ls_spa(method='subsets', groups=)`` returns; ``theta`` [p] and ``r_squared`` the full model's;
    ``baseline_r_squared`` the out-of-sample R^2 of the baseline columns alone (0 without a baseline).  The entries of
    ``attribution`` of group k sum to ``group_attribution[k]``, all of them to ``r_squared - baseline_r_squared``."""
    attribution: np.ndarray
    group_attribution: np.ndarray
    theta: np.ndarray
    r_squared: float
    baseline_r_squared: float

    def __repr__(self):
        pad = " " * 8
        lines = [
            "",
            f"{pad}p = {len(self.attribution)} columns in g = {len(self.group_attribution)} groups",
            f"{pad}Out-of-sample R^2 with all columns: {self.r_squared:.2e}",
            f"{pad}Out-of-sample R^2 of the baseline: {self.baseline_r_squared:.2e}",
            "",
            f"{pad}Shapley attribution of the groups: {_head(self.group_attribution)}",
            f"{pad}Owen values of the columns: {_head(self.attribution)}",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class BestSubsetsResults:
    """What ``ls_spa_best_subsets`` returns for p features and n = p + 1 - len(include) sizes.  ``sizes`` [n]: the
    model sizes len(include) .. p; ``subsets`` [n][p] bool: the best subset of each size (row i has ``sizes[i]`` True
    entries, the columns of ``include`` among them); ``r_squared`` [n]: its out-of-sample R^2; ``theta`` [n][p]: its
    coefficients, exactly 0.0 outside the subset.  A size without a candidate (every subset of that size had a Gram
    matrix that is not numerically positive definite) is a row of NaN in ``r_squared`` and ``theta`` and of False in
    ``subsets``.  ``best_size``: the size with the largest ``r_squared``, the smallest such size on ties, NaN sizes
    skipped (-1 if every size is NaN); ``best_subset`` [p] bool: its subset; ``full_r_squared``: the R^2 of all p
    features, what ``ls_spa(method='subsets').r_squared`` returns."""
    sizes: np.ndarray
    subsets: np.ndarray
    r_squared: np.ndarray
    theta: np.ndarray
    best_size: int
    best_subset: np.ndarray
    full_r_squared: float

    def __repr__(self):
        pad = " " * 8
        p = np.asarray(self.subsets).shape[1]
        chosen = ", ".join(str(j) for j in np.nonzero(self.best_subset)[0][:12])
        best = (f"{float(self.r_squared[self.best_size - int(self.sizes[0])]):.2e}"
                if self.best_size >= 0 else "nan")
        lines = [
            "",
            f"{pad}p = {p}, best subsets of sizes {int(self.sizes[0])} .. {int(self.sizes[-1])}",
            f"{pad}Out-of-sample R^2 with all features: {self.full_r_squared:.2e}",
            f"{pad}Best model: {self.best_size} features, out-of-sample R^2 {best}",
            f"{pad}Its features: ({chosen}{', ...' if int(np.sum(self.best_subset)) > 12 else ''})",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class TopSubsetsResults:
    """What ``ls_spa_top_subsets`` returns for p features, n = p + 1 - len(include) sizes and T = n_best ranks.
    ``sizes`` [n]: the model sizes len(include) .. p; ``n_models`` [n]: how many ranks of a size are valid, min(T, the
    number of subsets of that size that contain ``include``) unless subsets were dropped for a Gram matrix that is not
    numerically positive definite; ``subsets`` [n][T][p] bool: rank r of size i, best first -- the larger R^2, on equal
    values the subset with the smaller mask (bit j = feature j); ``r_squared`` [n][T]: its out-of-sample R^2,
    descending along a row; ``theta`` [n][T][p]: its coefficients, exactly 0.0 outside the subset; ``gap`` [n][T]:
    ``r_squared[:, :1] - r_squared``, what choosing rank r instead of the winner of its size costs.  Ranks past
    ``n_models`` are NaN in ``r_squared``, ``theta`` and ``gap`` and False in ``subsets``.  ``top_sizes`` [m],
    ``top_subsets`` [m][p] bool, ``top_r_squared`` [m]: the m = min(T, all valid ranks) best models over all sizes,
    in the same order.  ``best_size``, ``best_subset`` and ``full_r_squared`` are ``ls_spa_best_subsets``'s."""
    sizes: np.ndarray
    n_models: np.ndarray
    subsets: np.ndarray
    r_squared: np.ndarray
    theta: np.ndarray
    gap: np.ndarray
    top_sizes: np.ndarray
    top_subsets: np.ndarray
    top_r_squared: np.ndarray
    best_size: int
    best_subset: np.ndarray
    full_r_squared: float

    def __repr__(self):
        pad = " " * 8
        n, T, p = np.asarray(self.subsets).shape
        chosen = ", ".join(str(j) for j in np.nonzero(self.best_subset)[0][:12])
        best = runner = "nan"
        if self.best_size >= 0:
            best = f"{float(self.top_r_squared[0]):.2e}"
        if len(self.top_r_squared) > 1:
            runner = f"{float(self.top_r_squared[0] - self.top_r_squared[1]):.2e}"
        lines = [
            "",
            f"{pad}p = {p}, the {T} best subsets of sizes {int(self.sizes[0])} .. {int(self.sizes[-1])}",
            f"{pad}Out-of-sample R^2 with all features: {self.full_r_squared:.2e}",
            f"{pad}Best model: {self.best_size} features, out-of-sample R^2 {best}",
            f"{pad}Its features: ({chosen}{', ...' if int(np.sum(self.best_subset)) > 12 else ''})",
            f"{pad}The next model over all sizes is worse by {runner}",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class BestGroupSubsetsResults:
    """What ``ls_spa_best_subsets(groups=)`` returns for g groups over p columns: n = g + 1 sizes.  ``sizes`` [n]: 0 ..
    g, the number of groups in the model beside the baseline; ``group_subsets`` [n][g] bool: the best set of groups of
    each size (row i has ``sizes[i]`` True entries); ``subsets`` [n][p] bool: its columns, the baseline's (label -1)
    and the winning groups'; ``n_columns`` [n]: how many those are; ``r_squared`` [n]: its out-of-sample R^2;
    ``theta`` [n][p]: its coefficients, exactly 0.0 outside its columns.  A size without a candidate (every subset of
    that size had a Gram matrix that is not numerically positive definite) is a row of NaN in ``r_squared`` and
    ``theta``, of False in ``group_subsets`` and ``subsets`` and 0 in ``n_columns``.  ``best_size``: the size with the
    largest ``r_squared``, the smallest such size on ties, NaN sizes skipped (-1 if every size is NaN);
    ``best_group_subset`` [g] bool and ``best_subset`` [p] bool: its groups and its columns; ``full_r_squared``: the
    R^2 of all p columns, what ``ls_spa(method='subsets', groups=).r_squared`` returns; ``baseline_r_squared``: the R^2
    of the baseline alone, ``r_squared[0]`` (0.0 without a baseline)."""
    sizes: np.ndarray
    group_subsets: np.ndarray
    subsets: np.ndarray
    n_columns: np.ndarray
    r_squared: np.ndarray
    theta: np.ndarray
    best_size: int
    best_group_subset: np.ndarray
    best_subset: np.ndarray
    full_r_squared: float
    baseline_r_squared: float

    def __repr__(self):
        pad = " " * 8
        n, g = np.asarray(self.group_subsets).shape
        p = np.asarray(self.subsets).shape[1]
        chosen = ", ".join(str(k) for k in np.nonzero(self.best_group_subset)[0][:12])
        best = f"{float(self.r_squared[self.best_size]):.2e}" if self.best_size >= 0 else "nan"
        lines = [
            "",
            f"{pad}p = {p} columns in g = {g} groups, best group subsets of sizes 0 .. {n - 1}",
            f"{pad}Out-of-sample R^2 with all columns: {self.full_r_squared:.2e}, with the baseline alone: "
            f"{self.baseline_r_squared:.2e}",
            f"{pad}Best model: {self.best_size} groups ({int(np.sum(self.best_subset))} columns), out-of-sample R^2 "
            f"{best}",
            f"{pad}Its groups: ({chosen}{', ...' if int(np.sum(self.best_group_subset)) > 12 else ''})",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class TopGroupSubsetsResults:
    """What ``ls_spa_top_group_subsets`` returns for g groups over p columns, n = g + 1 sizes and T = n_best ranks.
    ``sizes`` [n]: 0 .. g, the number of groups in a model beside the baseline; ``n_models`` [n]: how many ranks of a
    size are valid, min(T, C(g, size)) unless group subsets were dropped for a Gram matrix that is not numerically
    positive definite; ``group_subsets`` [n][T][g] bool: rank r of size i, best first -- the larger R^2, on equal values
    the set with the smaller mask (bit k = group k); ``subsets`` [n][T][p] bool: its columns, the baseline's (label -1)
    and its groups'; ``n_columns`` [n][T]: how many those are; ``r_squared`` [n][T]: its out-of-sample R^2, descending
    along a row; ``theta`` [n][T][p]: its coefficients, exactly 0.0 outside its columns; ``gap`` [n][T]:
    ``r_squared[:, :1] - r_squared``, what choosing rank r instead of the winner of its size costs.  Ranks past
    ``n_models`` are NaN in ``r_squared``, ``theta`` and ``gap``, False in ``group_subsets`` and ``subsets`` and 0 in
    ``n_columns``.  ``top_sizes`` [m], ``top_group_subsets`` [m][g] bool, ``top_subsets`` [m][p] bool,
    ``top_r_squared`` [m]: the m = min(T, all valid ranks) best models over all sizes, in the same order.
    ``best_size``, ``best_group_subset``, ``best_subset``, ``full_r_squared`` and ``baseline_r_squared`` are
    ``ls_spa_best_subsets(groups=)``'s."""
    sizes: np.ndarray
    n_models: np.ndarray
    group_subsets: np.ndarray
    subsets: np.ndarray
    n_columns: np.ndarray
    r_squared: np.ndarray
    theta: np.ndarray
    gap: np.ndarray
    top_sizes: np.ndarray
    top_group_subsets: np.ndarray
    top_subsets: np.ndarray
    top_r_squared: np.ndarray
    best_size: int
    best_group_subset: np.ndarray
    best_subset: np.ndarray
    full_r_squared: float
    baseline_r_squared: float

    def __repr__(self):
        pad = " " * 8
        n, T, g = np.asarray(self.group_subsets).shape
        p = np.asarray(self.subsets).shape[2]
        chosen = ", ".join(str(k) for k in np.nonzero(self.best_group_subset)[0][:12])
        best = runner = "nan"
        if self.best_size >= 0:
            best = f"{float(self.top_r_squared[0]):.2e}"
        if len(self.top_r_squared) > 1:
            runner = f"{float(self.top_r_squared[0] - self.top_r_squared[1]):.2e}"
        lines = [
            "",
            f"{pad}p = {p} columns in g = {g} groups, the {T} best group subsets of sizes 0 .. {n - 1}",
            f"{pad}Out-of-sample R^2 with all columns: {self.full_r_squared:.2e}, with the baseline alone: "
            f"{self.baseline_r_squared:.2e}",
            f"{pad}Best model: {self.best_size} groups ({int(np.sum(self.best_subset))} columns), out-of-sample R^2 "
            f"{best}",
            f"{pad}Its groups: ({chosen}{', ...' if int(np.sum(self.best_group_subset)) > 12 else ''})",
            f"{pad}The next model over all sizes is worse by {runner}",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class PermutationTestResults:
    """What ``ls_spa_permutation_test`` returns; d = p, or the g groups of ``groups=``.  ``attribution`` [d], ``theta``
    [p], ``r_squared`` (and ``baseline_r_squared`` with groups, else None): the observed values.  ``null_attribution``
    [n_perm][d], ``null_r_squared`` [n_perm] (and ``null_baseline_r_squared`` [n_perm] with groups): the same under
    permutations of y; a null row sums to its ``null_r_squared`` (minus its baseline's with groups).  With n_valid the
    replicates that are finite (``n_failed`` = n_perm - n_valid):
    ``p_values`` [d] = (1 + #{r : null_attribution[r][j] >= attribution[j]}) / (1 + n_valid), one-sided;
    ``p_values_adjusted`` [d] = (1 + #{r : max_k null_attribution[r][k] >= attribution[j]}) / (1 + n_valid), single-step
    max-T: family-wise error control over the d players;
    ``r_squared_p_value`` the same from ``null_r_squared``."""
    attribution: np.ndarray
    theta: np.ndarray
    r_squared: float
    null_attribution: np.ndarray
    null_r_squared: np.ndarray
    p_values: np.ndarray
    p_values_adjusted: np.ndarray
    r_squared_p_value: float
    n_perm: int
    n_failed: int
    baseline_r_squared: float | None = None
    null_baseline_r_squared: np.ndarray | None = None

    @classmethod
    def from_null(cls, attribution, theta, r_squared, null_attribution, null_r_squared, baseline_r_squared=None,
                  null_baseline_r_squared=None):
        att, null = np.asarray(attribution, dtype=np.float64), np.asarray(null_attribution, dtype=np.float64)
        null_r2 = np.asarray(null_r_squared, dtype=np.float64)
        valid = np.isfinite(null).all(axis=1) & np.isfinite(null_r2)
        if null_baseline_r_squared is not None:
            valid &= np.isfinite(null_baseline_r_squared)
        n_valid = int(valid.sum())
        ok = null[valid]
        top = ok.max(axis=1) if ok.size else np.empty(0)
        return cls(
            attribution=att, theta=theta, r_squared=float(r_squared), null_attribution=null, null_r_squared=null_r2,
            p_values=(1 + (ok >= att[None, :]).sum(axis=0)) / (1 + n_valid),
            p_values_adjusted=(1 + (top[:, None] >= att[None, :]).sum(axis=0)) / (1 + n_valid),
            r_squared_p_value=float((1 + int((null_r2[valid] >= r_squared).sum())) / (1 + n_valid)),
            n_perm=len(null), n_failed=len(null) - n_valid,
            baseline_r_squared=None if baseline_r_squared is None else float(baseline_r_squared),
            null_baseline_r_squared=null_baseline_r_squared)

    def __repr__(self):
        pad = " " * 8
        lines = [
            "",
            f"{pad}d = {len(self.attribution)} players, n_perm = {self.n_perm} ({self.n_failed} failed)",
            f"{pad}Out-of-sample R^2 with all features: {self.r_squared:.2f} (p = {self.r_squared_p_value:.3g})",
            "",
            f"{pad}Shapley attribution: {_head(self.attribution)}",
            f"{pad}p-values: {_head(self.p_values)}",
            f"{pad}p-values, max-T adjusted: {_head(self.p_values_adjusted)}",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class SampledMultiResults:
    """What ``ls_spa_multi_sampled`` returns for m responses on one design matrix.  ``attribution`` [m][p]: row r is the
    mean of the ``n_samples`` lift vectors of response r, an estimate of its Shapley attribution; ``attribution_errors``
    [m][p] the standard errors of those means, sqrt(M2 / (n (n - 1))), ``inf`` while n < 2.  They assume independent
    samples: they are only indicative for the QMC sources ('argsort', 'permutohedron'), whose orderings are not
    independent, and for a caller's ``perms``.  ``theta`` [m][p] the full-model coefficients of each response;
    ``r_squared`` [m] their out-of-sample R^2 -- every sample's lifts telescope to it, so row r of ``attribution`` sums to
    ``r_squared[r]``."""
    attribution: np.ndarray
    attribution_errors: np.ndarray
    theta: np.ndarray
    r_squared: np.ndarray
    n_samples: int

    def __repr__(self):
        pad = " " * 8
        att = np.asarray(self.attribution)
        lines = [
            "",
            f"{pad}p = {att.shape[1]}, m = {att.shape[0]} responses, {self.n_samples} samples",
            f"{pad}Out-of-sample R^2 with all features: {_head(self.r_squared)}",
            "",
            f"{pad}Shapley attribution of response 0: {_head(att[0])}",
            f"{pad}Largest standard error: {float(np.max(self.attribution_errors)):.3g}",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class SampledCVResults:
    """What ``ls_spa_cv_sampled`` returns.  ``attribution`` [p]: the mean of the ``n_samples`` summed lift vectors
    sum_f lift_f(pi), an estimate of the Shapley attribution of the K-fold cross-validated R^2 (what ``ls_spa_cv`` gives
    exactly for p <= 32); ``attribution_errors`` [p] the standard errors of the SUMMED attribution, sqrt(M2 / (n (n - 1)))
    of the sums (``inf`` while n < 2; only indicative for the QMC sources and a caller's ``perms``).
    ``fold_attribution`` [K][p] and ``fold_attribution_errors`` [K][p]: the same per fold; the rows of
    ``fold_attribution`` sum to ``attribution``.  ``r_squared``: the cross-validated R^2 of the full model, what
    ``attribution`` sums to; ``fold_r_squared`` [K] each fold's share.  ``theta`` [p] is fitted on all rows;
    ``fold_ids`` [N] the fold of every row."""
    attribution: np.ndarray
    attribution_errors: np.ndarray
    fold_attribution: np.ndarray
    fold_attribution_errors: np.ndarray
    r_squared: float
    fold_r_squared: np.ndarray
    theta: np.ndarray
    fold_ids: np.ndarray
    n_samples: int

    def __repr__(self):
        pad = " " * 8
        lines = [
            "",
            f"{pad}p = {len(self.attribution)}, K = {len(self.fold_r_squared)} folds, {self.n_samples} samples",
            f"{pad}Cross-validated R^2 with all features: {self.r_squared:.6g}",
            "",
            f"{pad}Shapley attribution: {_head(self.attribution)}",
            f"{pad}Largest standard error: {float(np.max(self.attribution_errors)):.3g}",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class SampledCVGroupResults:
    """What ``ls_spa_cv_sampled(groups=)`` returns: ``SampledCVResults`` over the g groups -- ``attribution`` [g],
    ``attribution_errors`` [g], ``fold_attribution`` [K][g], ``fold_attribution_errors`` [K][g] -- with
    ``baseline_r_squared``, the cross-validated R^2 of the baseline's columns alone (0 without a baseline), and
    ``fold_baseline_r_squared`` [K] its shares.  ``attribution`` sums to ``r_squared - baseline_r_squared``; ``theta``
    keeps length p."""
    attribution: np.ndarray
    attribution_errors: np.ndarray
    fold_attribution: np.ndarray
    fold_attribution_errors: np.ndarray
    r_squared: float
    fold_r_squared: np.ndarray
    baseline_r_squared: float
    fold_baseline_r_squared: np.ndarray
    theta: np.ndarray
    fold_ids: np.ndarray
    n_samples: int

    def __repr__(self):
        pad = " " * 8
        lines = [
            "",
            f"{pad}g = {len(self.attribution)} groups, p = {len(self.theta)}, K = {len(self.fold_r_squared)} folds, "
            f"{self.n_samples} samples",
            f"{pad}Cross-validated R^2 with all columns: {self.r_squared:.6g}",
            f"{pad}Cross-validated R^2 of the baseline: {self.baseline_r_squared:.6g}",
            "",
            f"{pad}Shapley attribution: {_head(self.attribution)}",
            f"{pad}Largest standard error: {float(np.max(self.attribution_errors)):.3g}",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class SampledMultiGroupResults:
    """What ``ls_spa_multi_sampled(groups=)`` returns for m responses on one design matrix whose columns form g groups.
    ``attribution`` [m][g]: row r is the mean of the ``n_samples`` group lift vectors of response r, an estimate of its
    Shapley attribution over the groups (what ``ls_spa_groups`` estimates for that column alone);
    ``attribution_errors`` [m][g] the standard errors of those means, sqrt(M2 / (n (n - 1))), ``inf`` while n < 2 and
    only indicative where the samples are not independent (the QMC sources, a caller's ``perms``).  ``theta`` [m][p] the
    full-model coefficients of each response; ``r_squared`` [m] their out-of-sample R^2 and ``baseline_r_squared`` [m]
    that of the baseline columns alone (0 without a baseline) -- every sample's group lifts telescope from the one to
    the other, so row r of ``attribution`` sums to ``r_squared[r] - baseline_r_squared[r]``."""
    attribution: np.ndarray
    attribution_errors: np.ndarray
    theta: np.ndarray
    r_squared: np.ndarray
    baseline_r_squared: np.ndarray
    n_samples: int

    def __repr__(self):
        pad = " " * 8
        att = np.asarray(self.attribution)
        lines = [
            "",
            f"{pad}g = {att.shape[1]} groups, p = {np.asarray(self.theta).shape[1]}, m = {att.shape[0]} responses, "
            f"{self.n_samples} samples",
            f"{pad}Out-of-sample R^2 with all columns: {_head(self.r_squared)}",
            f"{pad}Out-of-sample R^2 of the baseline: {_head(self.baseline_r_squared)}",
            "",
            f"{pad}Shapley attribution of response 0: {_head(att[0])}",
            f"{pad}Largest standard error: {float(np.max(self.attribution_errors)):.3g}",
            pad,
        ]
        return "\n".join(lines)


class SizeIncompatible(Exception):
    """Raised when the shapes of the four data arrays do not fit together."""

    def __init__(self, message):
        self.message = message
        super().__init__(self.message)


_CHECKS = (
    (lambda Xa, Xe, ya, ye: Xa.shape[1] != Xe.shape[1],
     "X_train and X_test should have the same number of columns (features)."),
    (lambda Xa, Xe, ya, ye: Xa.shape[0] != ya.shape[0],
     "X_train should have the same number of rows as y_train has entries (observations)."),
    (lambda Xa, Xe, ya, ye: Xe.shape[0] != ye.shape[0],
     "X_test should have the same number of rows as y_test has entries (observations)."),
    (lambda Xa, Xe, ya, ye: Xa.shape[1] > Xa.shape[0],
     "The function works only if the number of features is at most the number of observations."),
)


def validate_data(X_train, X_test, y_train, y_test):
    for broken, message in _CHECKS:
        if broken(X_train, X_test, y_train, y_test):
            raise SizeIncompatible(message)


@dataclass
class BootstrapResults:
    """What ``ls_spa_bootstrap`` returns.  ``attribution``, ``theta`` and ``r_squared`` are the point estimate on the
    original rows, exactly those of ``ls_spa(method='subsets')``.  ``replicates`` [n_boot][p] and
    ``r_squared_replicates`` [n_boot] are the bootstrap replicates; a replicate whose Gram matrix was not numerically
    positive definite is NaN in both and counted in ``n_failed``.  Over the valid replicates: ``std_error`` [p] (sample
    standard deviation), ``lower`` / ``upper`` [p] and ``r_squared_interval`` (percentile interval: ``np.quantile`` at alpha =
    (1 - ``confidence``) / 2 and 1 - alpha, numpy's default interpolation) and ``prob_greater`` [p][p], the share of replicates with phi_i > phi_j.

    With ``groups=`` the players are the g groups: ``attribution``, ``replicates`` [n_boot][g], ``std_error``, ``lower``,
    ``upper`` have length g and ``prob_greater`` is [g][g] ("is variable A really worth more than variable B?");
    ``theta`` keeps length p.  A replicate's attribution then sums to its R^2 minus the R^2 of its baseline columns
    alone, ``baseline_r_squared_replicates`` [n_boot] (zeros without a baseline; None without ``groups=``)."""
    attribution: np.ndarray
    theta: np.ndarray
    r_squared: float
    replicates: np.ndarray
    r_squared_replicates: np.ndarray
    std_error: np.ndarray
    lower: np.ndarray
    upper: np.ndarray
    r_squared_interval: tuple
    n_failed: int
    prob_greater: np.ndarray
    confidence: float = 0.95
    baseline_r_squared_replicates: np.ndarray | None = None

    @classmethod
    def from_replicates(cls, attribution, theta, r_squared, replicates, r_squared_replicates, failed, confidence=0.95,
                        baseline_r_squared_replicates=None):
        """The summary fields from the replicates; failed [n_boot]: which replicates to mask.  RuntimeError when more
        than half of them failed."""
        rep = np.array(replicates, dtype=np.float64)
        r2 = np.array(r_squared_replicates, dtype=np.float64)
        failed = np.asarray(failed, dtype=bool)
        rep[failed] = np.nan
        r2[failed] = np.nan
        base = None
        if baseline_r_squared_replicates is not None:
            base = np.array(baseline_r_squared_replicates, dtype=np.float64)
            base[failed] = np.nan
        n_failed = int(failed.sum())
        if 2 * n_failed > len(rep):
            raise RuntimeError(f"{n_failed} of {len(rep)} bootstrap replicates had a Gram matrix that was not numerically "
                               "positive definite: no interval can be read from the rest")
        ok = rep[~failed]
        alpha = (1.0 - float(confidence)) / 2.0      # the interval is [quantile(alpha), quantile(1 - alpha)]
        lower, upper = np.quantile(ok, alpha, axis=0), np.quantile(ok, 1.0 - alpha, axis=0)
        r2_ok = r2[~failed]
        return cls(attribution=np.asarray(attribution), theta=np.asarray(theta), r_squared=float(r_squared),
                   replicates=rep, r_squared_replicates=r2,
                   std_error=ok.std(axis=0, ddof=1) if len(ok) > 1 else np.full(rep.shape[1], np.nan),
                   lower=lower, upper=upper,
                   r_squared_interval=(float(np.quantile(r2_ok, alpha)), float(np.quantile(r2_ok, 1.0 - alpha))),
                   n_failed=n_failed, prob_greater=(ok[:, :, None] > ok[:, None, :]).mean(axis=0),
                   confidence=float(confidence), baseline_r_squared_replicates=base)

    def __repr__(self):
        pad = " " * 8
        lines = [
            "",
            f"{pad}p = {np.asarray(self.attribution).size}, {len(self.replicates)} bootstrap replicates"
            + (f" ({self.n_failed} failed)" if self.n_failed else ""),
            f"{pad}Out-of-sample R^2 with all features: {self.r_squared:.2f}"
            f" [{self.r_squared_interval[0]:.2f}, {self.r_squared_interval[1]:.2f}]",
            "",
            f"{pad}Shapley attribution: {_head(self.attribution)}",
            f"{pad}{100 * self.confidence:g} % interval, lower: {_head(self.lower)}",
            f"{pad}{100 * self.confidence:g} % interval, upper: {_head(self.upper)}",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class SampledBootstrapResults:
    """What ``ls_spa_bootstrap_sampled`` returns.  ``attribution`` [d] and ``attribution_errors`` [d]: the point estimate
    on the original rows -- the mean of the ``n_samples`` lift vectors -- and its Monte-Carlo standard error
    sqrt(M2 / (n (n - 1))).  ``replicates`` [n_boot][d] and ``replicate_errors`` [n_boot][d]: each bootstrap replicate's
    mean lift over the SAME samples and its Monte-Carlo standard error; since the orderings are shared, their error
    moves all replicates together instead of widening their spread.  A replicate whose Gram matrix was not numerically
    positive definite in some ordering is NaN in ``replicates``, ``replicate_errors`` and ``r_squared_replicates`` and
    counted in ``n_failed``.  ``std_error``, ``lower``, ``upper``, ``prob_greater`` [d][d], ``r_squared_interval``:
    computed from ``replicates`` exactly as ``BootstrapResults`` computes them.  ``theta`` [p] and ``r_squared`` are the
    fit on the original rows."""
    attribution: np.ndarray
    attribution_errors: np.ndarray
    theta: np.ndarray
    r_squared: float
    replicates: np.ndarray
    replicate_errors: np.ndarray
    r_squared_replicates: np.ndarray
    std_error: np.ndarray
    lower: np.ndarray
    upper: np.ndarray
    r_squared_interval: tuple
    prob_greater: np.ndarray
    n_samples: int
    n_failed: int
    confidence: float = 0.95

    def _lines(self, what):
        pad = " " * 8
        return [
            "",
            f"{pad}{what}, {len(self.replicates)} bootstrap replicates"
            + (f" ({self.n_failed} failed)" if self.n_failed else "") + f", {self.n_samples} shared samples",
            f"{pad}Out-of-sample R^2 with all features: {self.r_squared:.2f}"
            f" [{self.r_squared_interval[0]:.2f}, {self.r_squared_interval[1]:.2f}]",
            "",
            f"{pad}Shapley attribution: {_head(self.attribution)}",
            f"{pad}Largest Monte-Carlo standard error: {float(np.max(self.attribution_errors)):.3g}",
            f"{pad}{100 * self.confidence:g} % interval, lower: {_head(self.lower)}",
            f"{pad}{100 * self.confidence:g} % interval, upper: {_head(self.upper)}",
            pad,
        ]

    def __repr__(self):
        return "\n".join(self._lines(f"p = {np.asarray(self.attribution).size}"))


@dataclass
class SampledBootstrapGroupResults(SampledBootstrapResults):
    """What ``ls_spa_bootstrap_sampled(groups=)`` returns: ``SampledBootstrapResults`` over the g groups, with
    ``baseline_r_squared``, the R^2 of the baseline's columns alone on the original rows (0 without a baseline), and
    ``baseline_r_squared_replicates`` [n_boot].  ``attribution`` sums to ``r_squared - baseline_r_squared`` and a
    replicate to its R^2 minus its baseline's; ``theta`` keeps length p."""
    baseline_r_squared: float = 0.0
    baseline_r_squared_replicates: np.ndarray | None = None

    def __repr__(self):
        return "\n".join(self._lines(f"g = {np.asarray(self.attribution).size} groups, p = {len(self.theta)}"))


@dataclass
class InteractionBootstrapResults:
    """What ``ls_spa_interactions_bootstrap`` returns.  ``interactions`` [d][d], ``attribution``, ``theta`` and
    ``r_squared`` are the point estimate on the original rows, exactly those of ``ls_spa_interactions``; d is p, or g with
    ``groups=``.  ``replicates`` [n_boot][d][d] are the bootstrap replicates of the matrix in the same convention (SHAP's:
    symmetric, half the pairwise index off the diagonal, main effects on it, row i summing to
    ``attribution_replicates[r][i]``), ``attribution_replicates`` [n_boot][d] and ``r_squared_replicates`` [n_boot] those
    of the attribution and of R^2; a replicate whose Gram matrix was not numerically positive definite is NaN in all of
    them and counted in ``n_failed``.  Over the valid replicates, each [d][d]: ``std_error`` (sample standard
    deviation), ``lower`` / ``upper`` (percentile interval: ``np.quantile`` at alpha = (1 - ``confidence``) / 2 and
    1 - alpha, numpy's default interpolation) and ``prob_positive``, the share of replicates with Phi_ij > 0 ("is this
    interaction really negative?" -- a share near 0 says yes).  With ``groups=`` a replicate's matrix sums to its R^2 minus
    the R^2 of its baseline columns alone, ``baseline_r_squared_replicates`` [n_boot] (zeros without a baseline; None
    without ``groups=``), and ``theta`` keeps length p."""
    interactions: np.ndarray
    attribution: np.ndarray
    theta: np.ndarray
    r_squared: float
    replicates: np.ndarray
    attribution_replicates: np.ndarray
    r_squared_replicates: np.ndarray
    std_error: np.ndarray
    lower: np.ndarray
    upper: np.ndarray
    prob_positive: np.ndarray
    n_failed: int
    confidence: float = 0.95
    baseline_r_squared_replicates: np.ndarray | None = None

    @classmethod
    def from_replicates(cls, interactions, attribution, theta, r_squared, replicates, attribution_replicates,
                        r_squared_replicates, failed, confidence=0.95, baseline_r_squared_replicates=None):
        """The summary fields from the replicates (matrices already in SHAP's convention); failed [n_boot]: which
        replicates to mask.  RuntimeError when more than half of them failed."""
        rep = np.array(replicates, dtype=np.float64)
        att = np.array(attribution_replicates, dtype=np.float64)
        r2 = np.array(r_squared_replicates, dtype=np.float64)
        failed = np.asarray(failed, dtype=bool)
        rep[failed] = np.nan
        att[failed] = np.nan
        r2[failed] = np.nan
        base = None
        if baseline_r_squared_replicates is not None:
            base = np.array(baseline_r_squared_replicates, dtype=np.float64)
            base[failed] = np.nan
        n_failed = int(failed.sum())
        if 2 * n_failed > len(rep):
            raise RuntimeError(f"{n_failed} of {len(rep)} bootstrap replicates had a Gram matrix that was not numerically "
                               "positive definite: no interval can be read from the rest")
        ok = rep[~failed]
        alpha = (1.0 - float(confidence)) / 2.0      # the interval is [quantile(alpha), quantile(1 - alpha)]
        return cls(interactions=np.asarray(interactions), attribution=np.asarray(attribution), theta=np.asarray(theta),
                   r_squared=float(r_squared), replicates=rep, attribution_replicates=att, r_squared_replicates=r2,
                   std_error=ok.std(axis=0, ddof=1) if len(ok) > 1 else np.full(rep.shape[1:], np.nan),
                   lower=np.quantile(ok, alpha, axis=0), upper=np.quantile(ok, 1.0 - alpha, axis=0),
                   prob_positive=(ok > 0.0).mean(axis=0), n_failed=n_failed, confidence=float(confidence),
                   baseline_r_squared_replicates=base)

    def __repr__(self):
        pad = " " * 8
        inter = np.asarray(self.interactions)
        off = inter - np.diag(np.diag(inter))
        lines = [
            "",
            f"{pad}d = {np.asarray(self.attribution).size}, {len(self.replicates)} bootstrap replicates"
            + (f" ({self.n_failed} failed)" if self.n_failed else ""),
            f"{pad}Out-of-sample R^2 with all features: {self.r_squared:.2f}",
            "",
            f"{pad}Shapley attribution: {_head(self.attribution)}",
            f"{pad}Largest pairwise interaction: {float(np.abs(off).max()) if off.size else 0.0:.2E}",
            f"{pad}Largest standard error: {float(np.nanmax(self.std_error)) if np.size(self.std_error) else 0.0:.2E}",
            pad,
        ]
        return "\n".join(lines)


def best_sizes(sizes, r_squared):
    """Per row of r_squared [..., n], the size with the largest value: the first of equal maxima (the smallest size), NaN
    skipped, -1 for a row that is all NaN -- the rule of ``BestSubsetsResults.best_size``."""
    r2 = np.asarray(r_squared, dtype=np.float64)
    empty = np.isnan(r2).all(axis=-1)
    first = np.argmax(np.where(np.isnan(r2), -np.inf, r2), axis=-1)       # argmax takes the first of equal maxima
    return np.where(empty, -1, np.asarray(sizes)[first]).astype(np.int64)


@dataclass
class BestSubsetsBootstrapResults:
    """What ``ls_spa_best_subsets_bootstrap`` returns for p features, n = p + 1 - len(include) sizes and n_boot
    replicates.  The point estimate on the original rows is exactly ``ls_spa_best_subsets``'s: ``sizes`` [n],
    ``subsets`` [n][p] bool, ``r_squared`` [n], ``best_size``, ``best_subset`` [p] bool, ``full_r_squared``.  The
    replicates: ``subset_replicates`` [n_boot][n][p] bool, the best subset of every size on the resampled rows;
    ``r_squared_replicates`` [n_boot][n], its out-of-sample R^2 there (NaN for a size without a candidate);
    ``best_size_replicates`` [n_boot], by the rule of ``best_size`` (the smallest of the sizes with the largest R^2, NaN
    skipped, -1 where every size is NaN); ``full_r_squared_replicates`` [n_boot].  A replicate whose Gram matrix was
    not numerically positive definite is NaN, False and -1 in these and counted in ``n_failed``.  Over the valid
    replicates: ``inclusion_frequency`` [n][p], the share whose size-k winner holds feature j ("how often is feature 5
    in the best model of three features?"); ``best_inclusion_frequency`` [p], the same for each replicate's overall best
    model; ``best_size_frequency`` [n], the share whose best model has that size; ``reselected`` [n], the share whose
    size-k winner is the point estimate's."""
    sizes: np.ndarray
    subsets: np.ndarray
    r_squared: np.ndarray
    best_size: int
    best_subset: np.ndarray
    full_r_squared: float
    subset_replicates: np.ndarray
    r_squared_replicates: np.ndarray
    best_size_replicates: np.ndarray
    full_r_squared_replicates: np.ndarray
    inclusion_frequency: np.ndarray
    best_inclusion_frequency: np.ndarray
    best_size_frequency: np.ndarray
    reselected: np.ndarray
    n_failed: int

    @classmethod
    def from_replicates(cls, point, values, masks, found, full_r_squared_replicates, failed):
        """The replicate and summary fields from the engine's rows.  point: the ``BestSubsetsResults`` of the original
        rows; values, masks, found [n_boot][n]: every replicate's best value, mask (bit j = feature j) and found flag
        at the sizes of ``point.sizes``; failed [n_boot]: which replicates to mask.  RuntimeError when more than half of
        them failed."""
        sizes = np.asarray(point.sizes)
        p = np.asarray(point.subsets).shape[1]
        failed = np.asarray(failed, dtype=bool)
        ok_entry = np.asarray(found, dtype=bool) & ~failed[:, None]
        bits = ((np.asarray(masks).astype(np.int64)[:, :, None] >> np.arange(p)) & 1).astype(bool)
        sub = bits & ok_entry[:, :, None]
        r2 = np.where(ok_entry, np.asarray(values, dtype=np.float64), np.nan)
        full = np.where(failed, np.nan, np.asarray(full_r_squared_replicates, dtype=np.float64))
        n_failed = int(failed.sum())
        if 2 * n_failed > len(failed):
            raise RuntimeError(f"{n_failed} of {len(failed)} bootstrap replicates had a Gram matrix that was not "
                               "numerically positive definite: no interval can be read from the rest")
        best = best_sizes(sizes, r2)
        valid = ~failed
        n_valid = max(int(valid.sum()), 1)
        row = np.clip(best - int(sizes[0]), 0, len(sizes) - 1)
        best_sub = sub[np.arange(len(sub)), row] & (best >= 0)[:, None]
        same = ok_entry & (sub == np.asarray(point.subsets, dtype=bool)[None]).all(axis=2)
        return cls(sizes=sizes, subsets=np.asarray(point.subsets), r_squared=np.asarray(point.r_squared),
                   best_size=int(point.best_size), best_subset=np.asarray(point.best_subset),
                   full_r_squared=float(point.full_r_squared), subset_replicates=sub, r_squared_replicates=r2,
                   best_size_replicates=best, full_r_squared_replicates=full,
                   inclusion_frequency=sub[valid].sum(axis=0) / n_valid,
                   best_inclusion_frequency=best_sub[valid].sum(axis=0) / n_valid,
                   best_size_frequency=(best[valid][:, None] == sizes[None, :]).sum(axis=0) / n_valid,
                   reselected=same[valid].sum(axis=0) / n_valid, n_failed=n_failed)

    def __repr__(self):
        pad = " " * 8
        p = np.asarray(self.subsets).shape[1]
        chosen = np.nonzero(self.best_subset)[0]
        freq = ", ".join(f"{j}: {self.best_inclusion_frequency[j]:.2f}" for j in chosen[:12])
        lines = [
            "",
            f"{pad}p = {p}, {len(self.subset_replicates)} bootstrap replicates of the best subsets of sizes "
            f"{int(self.sizes[0])} .. {int(self.sizes[-1])}" + (f" ({self.n_failed} failed)" if self.n_failed else ""),
            f"{pad}Best model: {self.best_size} features, the best size in "
            f"{float(self.best_size_frequency[self.best_size - int(self.sizes[0])]) if self.best_size >= 0 else 0.0:.2f}"
            " of the replicates",
            f"{pad}Its features and how often a replicate's best model holds them: ({freq}"
            f"{', ...' if len(chosen) > 12 else ''})",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class BestGroupSubsetsBootstrapResults:
    """What ``ls_spa_best_group_subsets_bootstrap`` returns for g groups over p columns (sizes 0 .. g, n = g + 1) and
    n_boot replicates.  The point estimate on the original rows is exactly ``ls_spa_best_subsets(groups=)``'s: ``sizes``
    [n], ``group_subsets`` [n][g] bool, ``subsets`` [n][p] bool, ``r_squared`` [n], ``best_size``,
    ``best_group_subset`` [g] bool, ``best_subset`` [p] bool, ``full_r_squared``, ``baseline_r_squared``.  The
    replicates: ``group_subset_replicates`` [n_boot][n][g] bool, the best set of every number of groups on the resampled
    rows; ``r_squared_replicates`` [n_boot][n], its out-of-sample R^2 there (NaN for a size without a candidate);
    ``best_size_replicates`` [n_boot], by the rule of ``best_size`` (-1 where every size is NaN);
    ``full_r_squared_replicates`` and ``baseline_r_squared_replicates`` [n_boot], the R^2 of each replicate's full model
    and of its baseline columns alone.  A failed replicate (a Gram matrix that was not numerically positive definite) is
    NaN, False and -1 in these and counted in ``n_failed``.  Over the valid replicates, with the groups as the players
    of ``BestSubsetsBootstrapResults``: ``inclusion_frequency`` [n][g], the share whose size-k winner holds group j;
    ``best_inclusion_frequency`` [g], the same for each replicate's overall best model; ``best_size_frequency`` [n];
    ``reselected`` [n], the share whose size-k winner is the point estimate's."""
    sizes: np.ndarray
    group_subsets: np.ndarray
    subsets: np.ndarray
    r_squared: np.ndarray
    best_size: int
    best_group_subset: np.ndarray
    best_subset: np.ndarray
    full_r_squared: float
    baseline_r_squared: float
    group_subset_replicates: np.ndarray
    r_squared_replicates: np.ndarray
    best_size_replicates: np.ndarray
    full_r_squared_replicates: np.ndarray
    baseline_r_squared_replicates: np.ndarray
    inclusion_frequency: np.ndarray
    best_inclusion_frequency: np.ndarray
    best_size_frequency: np.ndarray
    reselected: np.ndarray
    n_failed: int

    @classmethod
    def from_replicates(cls, point, values, masks, found, full_r_squared_replicates, baseline_r_squared_replicates,
                        failed):
        """The replicate and summary fields from the engine's rows.  point: the ``BestGroupSubsetsResults`` of the
        original rows; values, masks, found [n_boot][g + 1]: every replicate's best value, mask (bit k = group k) and
        found flag; failed [n_boot]: which replicates to mask.  The tallies are
        ``BestSubsetsBootstrapResults.from_replicates``'s with the groups as the players; its RuntimeError when more
        than half of the replicates failed."""
        players = BestSubsetsResults(sizes=np.asarray(point.sizes), subsets=np.asarray(point.group_subsets),
                                     r_squared=np.asarray(point.r_squared), theta=None, best_size=int(point.best_size),
                                     best_subset=np.asarray(point.best_group_subset),
                                     full_r_squared=float(point.full_r_squared))
        t = BestSubsetsBootstrapResults.from_replicates(players, values, masks, found, full_r_squared_replicates, failed)
        base = np.where(np.asarray(failed, dtype=bool), np.nan,
                        np.asarray(baseline_r_squared_replicates, dtype=np.float64))
        return cls(sizes=t.sizes, group_subsets=t.subsets, subsets=np.asarray(point.subsets), r_squared=t.r_squared,
                   best_size=t.best_size, best_group_subset=t.best_subset, best_subset=np.asarray(point.best_subset),
                   full_r_squared=t.full_r_squared, baseline_r_squared=float(point.baseline_r_squared),
                   group_subset_replicates=t.subset_replicates, r_squared_replicates=t.r_squared_replicates,
                   best_size_replicates=t.best_size_replicates, full_r_squared_replicates=t.full_r_squared_replicates,
                   baseline_r_squared_replicates=base, inclusion_frequency=t.inclusion_frequency,
                   best_inclusion_frequency=t.best_inclusion_frequency, best_size_frequency=t.best_size_frequency,
                   reselected=t.reselected, n_failed=t.n_failed)

    def __repr__(self):
        pad = " " * 8
        g = np.asarray(self.group_subsets).shape[1]
        chosen = np.nonzero(self.best_group_subset)[0]
        freq = ", ".join(f"{j}: {self.best_inclusion_frequency[j]:.2f}" for j in chosen[:12])
        lines = [
            "",
            f"{pad}g = {g} groups over p = {np.asarray(self.subsets).shape[1]} columns, "
            f"{len(self.group_subset_replicates)} bootstrap replicates of the best sets of 0 .. {g} groups"
            + (f" ({self.n_failed} failed)" if self.n_failed else ""),
            f"{pad}Best model: {self.best_size} groups, the best size in "
            f"{float(self.best_size_frequency[self.best_size]) if self.best_size >= 0 else 0.0:.2f} of the replicates",
            f"{pad}Its groups and how often a replicate's best model holds them: ({freq}"
            f"{', ...' if len(chosen) > 12 else ''})",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class CVResults:
    """What ``ls_spa_cv`` returns for p features, K folds and N rows.  ``attribution`` [p]: the exact Shapley attribution
    of the K-fold cross-validated R^2; ``fold_attribution`` [K][p]: the folds' attributions, whose sum over the folds in
    ascending order it is; ``r_squared``: the cross-validated R^2 of the full model,
    1 - sum_f ||y_f - X_f theta^(-f)||^2 / ||y||^2, what ``attribution`` sums to; ``fold_r_squared`` [K]: each fold's
    share of it (over the pooled ||y||^2, so the shares add up to ``r_squared``); ``theta`` [p]: the coefficients fitted
    on all rows; ``fold_ids`` [N]: the fold of every row."""
    attribution: np.ndarray
    fold_attribution: np.ndarray
    r_squared: float
    fold_r_squared: np.ndarray
    theta: np.ndarray
    fold_ids: np.ndarray

    def __repr__(self):
        pad = " " * 8
        lines = [
            "",
            f"{pad}p = {len(self.attribution)}, {len(self.fold_r_squared)}-fold cross-validation",
            f"{pad}Cross-validated R^2: {self.r_squared:.2e}",
            f"{pad}Attribution: ({_head(self.attribution)})",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class CVBestSubsetsResults:
    """What ``ls_spa_best_subsets_cv`` returns for p features, K folds and n = p + 1 - len(include) sizes: the fields of
    ``BestSubsetsResults`` with the K-fold cross-validated R^2 as the value.  ``r_squared`` [n]: the winner's
    cross-validated value; ``fold_r_squared`` [n][K]: its per-fold values, whose sum in ascending fold order it is;
    ``theta`` [n][p]: the winner refitted on ALL rows, exactly 0.0 outside its subset; ``full_r_squared``: the
    cross-validated R^2 of all p columns; ``fold_ids`` [N]: the fold of every row.  A size without a candidate is a row
    of NaN / False, as there; ``best_size`` is the smallest size on ties, NaN rows skipped (-1 if every size is NaN)."""
    sizes: np.ndarray
    subsets: np.ndarray
    r_squared: np.ndarray
    fold_r_squared: np.ndarray
    theta: np.ndarray
    best_size: int
    best_subset: np.ndarray
    full_r_squared: float
    fold_ids: np.ndarray

    def __repr__(self):
        pad = " " * 8
        p = np.asarray(self.subsets).shape[1]
        chosen = ", ".join(str(j) for j in np.nonzero(self.best_subset)[0][:12])
        best = (f"{float(self.r_squared[self.best_size - int(self.sizes[0])]):.2e}"
                if self.best_size >= 0 else "nan")
        lines = [
            "",
            f"{pad}p = {p}, {np.asarray(self.fold_r_squared).shape[1]}-fold cross-validation, best subsets of sizes "
            f"{int(self.sizes[0])} .. {int(self.sizes[-1])}",
            f"{pad}Cross-validated R^2 with all features: {self.full_r_squared:.2e}",
            f"{pad}Best model: {self.best_size} features, cross-validated R^2 {best}",
            f"{pad}Its features: ({chosen}{', ...' if int(np.sum(self.best_subset)) > 12 else ''})",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class TopSubsetsCVResults:
    """What ``ls_spa_top_subsets_cv`` returns for p features, K folds, n = p + 1 - len(include) sizes and T = n_best
    ranks: the fields of ``TopSubsetsResults`` with the K-fold cross-validated R^2 as the value.  ``r_squared`` [n][T]:
    rank r of size i, best first -- the larger value, on equal values the subset with the smaller mask;
    ``fold_r_squared`` [n][T][K]: its per-fold values, whose sum in ascending fold order it is; ``theta`` [n][T][p]: the
    model refitted on ALL rows, exactly 0.0 outside its subset; ``gap`` [n][T]: ``r_squared[:, :1] - r_squared``;
    ``top_sizes``, ``top_subsets``, ``top_r_squared``: the min(T, all valid ranks) best models over all sizes;
    ``best_size``, ``best_subset``, ``full_r_squared``: ``ls_spa_best_subsets_cv``'s; ``fold_ids`` [N]: the fold of
    every row.  Ranks past ``n_models`` are NaN (False in ``subsets`` and ``within_one_se``).

    Against the overall best model b (rank 0 of ``best_size``), from ``fold_r_squared`` alone, with the paired per-fold
    differences d_f = fold_r_squared[b][f] - fold_r_squared[i, r][f]: ``best_gap`` [n][T] = r_squared[b] -
    r_squared[i, r]; ``best_gap_std_error`` [n][T] = sqrt(K) std(d, ddof=1); ``within_one_se`` [n][T] = best_gap <=
    best_gap_std_error; ``one_se_size``: the smallest size whose rank 0 is within one standard error (``best_size``
    always is; -1 if nothing is listed) and ``one_se_subset`` [p] bool, that size's rank 0.  K folds are few and their
    training sets overlap: this is the usual one-standard-error heuristic, not a test."""
    sizes: np.ndarray
    n_models: np.ndarray
    subsets: np.ndarray
    r_squared: np.ndarray
    fold_r_squared: np.ndarray
    theta: np.ndarray
    gap: np.ndarray
    top_sizes: np.ndarray
    top_subsets: np.ndarray
    top_r_squared: np.ndarray
    best_size: int
    best_subset: np.ndarray
    full_r_squared: float
    best_gap: np.ndarray
    best_gap_std_error: np.ndarray
    within_one_se: np.ndarray
    one_se_size: int
    one_se_subset: np.ndarray
    fold_ids: np.ndarray

    def __repr__(self):
        pad = " " * 8
        n, T, p = np.asarray(self.subsets).shape
        K = np.asarray(self.fold_r_squared).shape[2]
        chosen = ", ".join(str(j) for j in np.nonzero(self.best_subset)[0][:12])
        best = runner = "nan"
        if self.best_size >= 0:
            best = f"{float(self.top_r_squared[0]):.2e}"
        if len(self.top_r_squared) > 1:
            runner = f"{float(self.top_r_squared[0] - self.top_r_squared[1]):.2e}"
        lines = [
            "",
            f"{pad}p = {p}, {K}-fold cross-validation, the {T} best subsets of sizes {int(self.sizes[0])} .. "
            f"{int(self.sizes[-1])}",
            f"{pad}Cross-validated R^2 with all features: {self.full_r_squared:.2e}",
            f"{pad}Best model: {self.best_size} features, cross-validated R^2 {best}",
            f"{pad}Its features: ({chosen}{', ...' if int(np.sum(self.best_subset)) > 12 else ''})",
            f"{pad}The next model over all sizes is worse by {runner}",
            f"{pad}Smallest size within one standard error of the best: {self.one_se_size}; listed models within it: "
            f"{int(np.sum(self.within_one_se))}",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class CVGroupResults:
    """What ``ls_spa_cv(groups=)`` returns for g groups of p columns, K folds and N rows.  ``attribution`` [g]: the exact
    Shapley attribution of the K-fold cross-validated R^2 to the groups; ``fold_attribution`` [K][g]: the folds'
    attributions, whose sum over the folds in ascending order it is; ``r_squared``: the cross-validated R^2 of the full
    model; ``fold_r_squared`` [K]: each fold's share of it; ``baseline_r_squared``: the cross-validated R^2 of the
    baseline's columns alone (label -1; 0.0 without a baseline) and ``fold_baseline_r_squared`` [K] its shares --
    ``attribution`` sums to ``r_squared - baseline_r_squared``; ``theta`` [p]: the coefficients fitted on all rows;
    ``fold_ids`` [N]: the fold of every row."""
    attribution: np.ndarray
    fold_attribution: np.ndarray
    r_squared: float
    fold_r_squared: np.ndarray
    baseline_r_squared: float
    fold_baseline_r_squared: np.ndarray
    theta: np.ndarray
    fold_ids: np.ndarray

    def __repr__(self):
        pad = " " * 8
        lines = [
            "",
            f"{pad}g = {len(self.attribution)} groups of p = {len(self.theta)} columns, "
            f"{len(self.fold_r_squared)}-fold cross-validation",
            f"{pad}Cross-validated R^2: {self.r_squared:.2e} (baseline alone: {self.baseline_r_squared:.2e})",
            f"{pad}Attribution: ({_head(self.attribution)})",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class CVPathResults:
    """What ``ls_spa_cv_path`` returns for L ridge values, p features, K folds and N rows: row l of every field is
    ``ls_spa_cv(X, y, reg=regs[l])``'s, bit for bit.  ``regs`` [L]: the ridge values in the caller's order;
    ``attribution`` [L][p]; ``fold_attribution`` [L][K][p], whose sum over the folds in ascending order it is;
    ``r_squared`` [L]: the cross-validated R^2 of the full model, what a row of ``attribution`` sums to;
    ``fold_r_squared`` [L][K]: each fold's share of it; ``theta`` [L][p]: the coefficients fitted on all rows with that
    ridge value; ``fold_ids`` [N]: the fold of every row.

    ``best_index`` / ``best_reg``: the row of the largest ``r_squared``, on equal values the larger ridge value, NaN
    rows skipped (-1 / NaN if every row is NaN).  Against that row b, from ``fold_r_squared`` alone, with the paired
    per-fold differences d_f = fold_r_squared[b][f] - fold_r_squared[l][f]: ``best_gap`` [L] = their sum;
    ``best_gap_std_error`` [L] = sqrt(K) std(d, ddof=1); ``within_one_se`` [L] = best_gap <= best_gap_std_error (False
    in a NaN row); ``one_se_index`` / ``one_se_reg``: the largest ridge value within one standard error of the best
    (``best_index``'s own row always is).  K folds are few and their training sets overlap: this is the usual
    one-standard-error heuristic for preferring the stronger penalty, not a test."""
    regs: np.ndarray
    attribution: np.ndarray
    fold_attribution: np.ndarray
    r_squared: np.ndarray
    fold_r_squared: np.ndarray
    theta: np.ndarray
    fold_ids: np.ndarray
    best_index: int
    best_reg: float
    best_gap: np.ndarray
    best_gap_std_error: np.ndarray
    within_one_se: np.ndarray
    one_se_index: int
    one_se_reg: float

    def __repr__(self):
        pad = " " * 8
        L, p = np.asarray(self.attribution).shape
        best = f"{float(self.r_squared[self.best_index]):.2e}" if self.best_index >= 0 else "nan"
        lines = [
            "",
            f"{pad}p = {p}, {np.asarray(self.fold_r_squared).shape[1]}-fold cross-validation, {L} ridge values "
            f"{float(np.min(self.regs)):.2e} .. {float(np.max(self.regs)):.2e}",
            f"{pad}Best ridge value: {self.best_reg:.2e}, cross-validated R^2 {best}",
            f"{pad}Largest ridge value within one standard error of it: {self.one_se_reg:.2e}",
            f"{pad}Attribution at the best: ({_head(self.attribution[self.best_index]) if self.best_index >= 0 else ''})",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class CVGroupPathResults:
    """What ``ls_spa_cv_path(groups=)`` returns for L ridge values, g groups of p columns and K folds: the fields of
    ``CVPathResults`` over the groups -- ``attribution`` [L][g], ``fold_attribution`` [L][K][g], row l
    ``ls_spa_cv(X, y, reg=regs[l], groups=)``'s, bit for bit -- plus ``baseline_r_squared`` [L] (the cross-validated
    R^2 of the baseline's columns alone; a row of ``attribution`` sums to ``r_squared - baseline_r_squared``) and
    ``fold_baseline_r_squared`` [L][K].  The choice of the ridge value and the one-standard-error fields are those of
    ``CVPathResults``, from ``r_squared`` and ``fold_r_squared`` of the full model."""
    regs: np.ndarray
    attribution: np.ndarray
    fold_attribution: np.ndarray
    r_squared: np.ndarray
    fold_r_squared: np.ndarray
    baseline_r_squared: np.ndarray
    fold_baseline_r_squared: np.ndarray
    theta: np.ndarray
    fold_ids: np.ndarray
    best_index: int
    best_reg: float
    best_gap: np.ndarray
    best_gap_std_error: np.ndarray
    within_one_se: np.ndarray
    one_se_index: int
    one_se_reg: float

    def __repr__(self):
        pad = " " * 8
        L, g = np.asarray(self.attribution).shape
        best = f"{float(self.r_squared[self.best_index]):.2e}" if self.best_index >= 0 else "nan"
        lines = [
            "",
            f"{pad}g = {g} groups of p = {np.asarray(self.theta).shape[1]} columns, "
            f"{np.asarray(self.fold_r_squared).shape[1]}-fold cross-validation, {L} ridge values "
            f"{float(np.min(self.regs)):.2e} .. {float(np.max(self.regs)):.2e}",
            f"{pad}Best ridge value: {self.best_reg:.2e}, cross-validated R^2 {best}",
            f"{pad}Largest ridge value within one standard error of it: {self.one_se_reg:.2e}",
            f"{pad}Attribution at the best: ({_head(self.attribution[self.best_index]) if self.best_index >= 0 else ''})",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class CVBestGroupSubsetsResults:
    """What ``ls_spa_best_subsets_cv(groups=)`` returns for g groups of p columns and K folds: the fields of
    ``BestGroupSubsetsResults`` with the K-fold cross-validated R^2 as the value.  ``sizes``: 0 .. g (size 0 is the
    baseline alone); ``group_subsets`` [g + 1][g] bool; ``subsets`` [g + 1][p] bool (the baseline's and the winners'
    columns); ``n_columns`` [g + 1]; ``r_squared`` [g + 1]: the winner's cross-validated value; ``fold_r_squared``
    [g + 1][K]: its per-fold values, whose sum in ascending fold order it is; ``theta`` [g + 1][p]: the winner refitted
    on ALL rows, exactly 0.0 outside its columns; ``full_r_squared``: the cross-validated R^2 of all groups;
    ``baseline_r_squared``: ``r_squared[0]``; ``fold_ids`` [N].  A size without a candidate is a row of NaN / False;
    ``best_size`` is the smallest size on ties, NaN rows skipped (-1 if every size is NaN)."""
    sizes: np.ndarray
    group_subsets: np.ndarray
    subsets: np.ndarray
    n_columns: np.ndarray
    r_squared: np.ndarray
    fold_r_squared: np.ndarray
    theta: np.ndarray
    best_size: int
    best_group_subset: np.ndarray
    best_subset: np.ndarray
    full_r_squared: float
    baseline_r_squared: float
    fold_ids: np.ndarray

    def __repr__(self):
        pad = " " * 8
        g, p = np.asarray(self.group_subsets).shape[1], np.asarray(self.subsets).shape[1]
        chosen = ", ".join(str(j) for j in np.nonzero(self.best_group_subset)[0][:12])
        best = f"{float(self.r_squared[self.best_size]):.2e}" if self.best_size >= 0 else "nan"
        lines = [
            "",
            f"{pad}g = {g} groups of p = {p} columns, {np.asarray(self.fold_r_squared).shape[1]}-fold cross-validation, "
            f"best sets of groups of sizes 0 .. {g}",
            f"{pad}Cross-validated R^2 with all groups: {self.full_r_squared:.2e} (baseline alone: "
            f"{self.baseline_r_squared:.2e})",
            f"{pad}Best model: {self.best_size} groups, cross-validated R^2 {best}",
            f"{pad}Its groups: ({chosen}{', ...' if int(np.sum(self.best_group_subset)) > 12 else ''})",
            pad,
        ]
        return "\n".join(lines)


@dataclass
class TopGroupSubsetsCVResults:
    """What ``ls_spa_top_group_subsets_cv`` returns for g groups of p columns, K folds, n = g + 1 sizes and
    T = n_best ranks: the fields of ``TopGroupSubsetsResults`` with the K-fold cross-validated R^2 as the value.
    ``sizes`` [n]: 0 .. g (size 0 is the baseline alone); ``n_models`` [n]: the valid ranks of a size;
    ``group_subsets`` [n][T][g] bool: rank r of size i, best first -- the larger value, on equal values the set with the
    smaller mask (bit k = group k); ``subsets`` [n][T][p] bool: its columns, the baseline's and its groups';
    ``n_columns`` [n][T]; ``r_squared`` [n][T]; ``fold_r_squared`` [n][T][K]: its per-fold values, whose sum in
    ascending fold order it is; ``theta`` [n][T][p]: the model refitted on ALL rows, exactly 0.0 outside its columns;
    ``gap`` [n][T]: ``r_squared[:, :1] - r_squared``; ``top_sizes``, ``top_group_subsets``, ``top_subsets``,
    ``top_r_squared``: the min(T, all valid ranks) best models over all sizes; ``best_size``, ``best_group_subset``,
    ``best_subset``, ``full_r_squared``, ``baseline_r_squared``: ``ls_spa_best_subsets_cv(groups=)``'s; ``fold_ids``
    [N].  Ranks past ``n_models`` are NaN (False in the subsets and ``within_one_se``, 0 in ``n_columns``).

    ``best_gap``, ``best_gap_std_error``, ``within_one_se`` [n][T], ``one_se_size`` and ``one_se_subset`` are those of
    ``TopSubsetsCVResults``, against the overall best model (rank 0 of ``best_size``) from ``fold_r_squared`` alone;
    ``one_se_group_subset`` [g] bool: the groups of that size's rank 0.  The usual one-standard-error heuristic, not a
    test."""
    sizes: np.ndarray
    n_models: np.ndarray
    group_subsets: np.ndarray
    subsets: np.ndarray
    n_columns: np.ndarray
    r_squared: np.ndarray
    fold_r_squared: np.ndarray
    theta: np.ndarray
    gap: np.ndarray
    top_sizes: np.ndarray
    top_group_subsets: np.ndarray
    top_subsets: np.ndarray
    top_r_squared: np.ndarray
    best_size: int
    best_group_subset: np.ndarray
    best_subset: np.ndarray
    full_r_squared: float
    baseline_r_squared: float
    best_gap: np.ndarray
    best_gap_std_error: np.ndarray
    within_one_se: np.ndarray
    one_se_size: int
    one_se_group_subset: np.ndarray
    one_se_subset: np.ndarray
    fold_ids: np.ndarray

    def __repr__(self):
        pad = " " * 8
        n, T, g = np.asarray(self.group_subsets).shape
        p = np.asarray(self.subsets).shape[2]
        K = np.asarray(self.fold_r_squared).shape[2]
        chosen = ", ".join(str(k) for k in np.nonzero(self.best_group_subset)[0][:12])
        best = runner = "nan"
        if self.best_size >= 0:
            best = f"{float(self.top_r_squared[0]):.2e}"
        if len(self.top_r_squared) > 1:
            runner = f"{float(self.top_r_squared[0] - self.top_r_squared[1]):.2e}"
        lines = [
            "",
            f"{pad}g = {g} groups of p = {p} columns, {K}-fold cross-validation, the {T} best sets of groups of sizes "
            f"0 .. {n - 1}",
            f"{pad}Cross-validated R^2 with all groups: {self.full_r_squared:.2e} (baseline alone: "
            f"{self.baseline_r_squared:.2e})",
            f"{pad}Best model: {self.best_size} groups ({int(np.sum(self.best_subset))} columns), cross-validated R^2 "
            f"{best}",
            f"{pad}Its groups: ({chosen}{', ...' if int(np.sum(self.best_group_subset)) > 12 else ''})",
            f"{pad}The next model over all sizes is worse by {runner}",
            f"{pad}Smallest size within one standard error of the best: {self.one_se_size}; listed models within it: "
            f"{int(np.sum(self.within_one_se))}",
            pad,
        ]
        return "\n".join(lines)
