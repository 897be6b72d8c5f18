"""MI355X-native LS-SPA: a drop-in for the ``ls_spa`` package of cvxgrp/ls-spa.

Same public names as the reference's ``from .ls_spa import *`` (ls_spa/__init__.py:1):
``ls_spa``, ``ShapleyResults``, ``SizeIncompatible``, ``validate_data``,
``merge_sample_mean``, ``merge_sample_cov``, ``square_shapley``, ``reduce_data``,
``error_estimates``; ``ls_spa_groups`` (sampled attribution over groups of columns) and ``ls_spa_interactions`` (exact
pairwise Shapley interaction values between features, p <= 32, or between groups of columns, g <= 32) and
``ls_spa_interactions_sampled`` (their sampled counterpart, for any number of features or groups) and
``ls_spa_bootstrap`` (bootstrap confidence intervals of the exact attribution, p <= 32, or over g <= 32 groups of p <= 64 columns)
and ``ls_spa_interactions_bootstrap`` (the same for the exact interaction values) and ``ls_spa_multi`` (the exact
attribution of many responses on one design matrix, p <= 32, or with ``groups=`` over g <= 32 groups of p <= 64 columns,
returning ``MultiGroupResults``) and ``ls_spa_multi_sampled`` (the sampled attribution of many responses on one design
matrix, p <= 104, or with ``groups=`` over groups of those columns, returning ``SampledMultiGroupResults``) and
``ls_spa_permutation_test`` (permutation p-values for the exact attribution and R^2, p <= 32, or with ``groups=`` over
g <= 32 groups of p <= 64 columns) and ``ls_spa_owen`` (exact Owen values: the attribution of every column with
``groups=`` as coalition structure, returning ``OwenResults``) and ``ls_spa_best_subsets`` (exhaustive best-subset
selection: the best model of every size by out-of-sample R^2 over all 2^p subsets, p <= 32, returning
``BestSubsetsResults``, or with ``groups=`` over all 2^g sets of g <= 32 groups of p <= 64 columns, returning
``BestGroupSubsetsResults``) and ``ls_spa_best_subsets_bootstrap`` (the bootstrap of that selection, p <= 32: how often
each feature, each size and each winner is chosen again on resampled rows, returning ``BestSubsetsBootstrapResults``)
and ``ls_spa_best_group_subsets_bootstrap`` (the same over groups of columns, g <= 32 groups of p <= 64 columns: the
bootstrap of ``ls_spa_best_subsets(groups=)``, returning ``BestGroupSubsetsBootstrapResults``) and
``ls_spa_top_subsets`` (the n_best <= 16 best models of every size, p <= 32: how much worse is the next model?,
returning ``TopSubsetsResults``) and ``ls_spa_top_group_subsets`` (the same over groups of columns, g <= 32 groups of
p <= 64 columns: the n_best <= 16 best sets of groups of every size, returning ``TopGroupSubsetsResults``) and
``ls_spa_cv`` (the exact attribution of the K-fold cross-validated R^2 of one data set, p <= 32, returning
``CVResults``) and ``ls_spa_best_subsets_cv`` (best-subset selection by that cross-validated R^2, returning
``CVBestSubsetsResults``; ``cv_fold_ids`` is the fold assignment of both; with ``groups=`` both work on g <= 32 groups
of p <= 64 columns and return ``CVGroupResults`` and ``CVBestGroupSubsetsResults``) and ``ls_spa_top_subsets_cv`` (the
n_best <= 16 best models of every size by that cross-validated R^2, p <= 32, with the one-standard-error fields the
folds' paired values give, returning ``TopSubsetsCVResults``) and ``ls_spa_top_group_subsets_cv`` (the same over g <= 32
groups of p <= 64 columns, returning ``TopGroupSubsetsCVResults``) and ``ls_spa_cv_path`` (``ls_spa_cv`` for a path of
ridge values on one load, row by row its bits, with the choice of the value the folds prefer, returning
``CVPathResults``, with ``groups=`` ``CVGroupPathResults``) and ``ls_spa_cv_sampled`` (the sampled attribution of
that cross-validated R^2 for p <= 127, or with ``groups=`` over groups of those columns, returning ``SampledCVResults``
and ``SampledCVGroupResults``) and ``ls_spa_bootstrap_sampled`` (bootstrap confidence intervals for the sampled
attribution for p <= 127, all replicates on one shared set of orderings, returning ``SampledBootstrapResults``, with
``groups=`` ``SampledBootstrapGroupResults``)
are this package's own.  Every ordering is evaluated by hand-written HIP kernels for gfx950
behind a C ABI (include/lsspa.h); there is no CPU fallback.
"""
from ._results import (CVBestGroupSubsetsResults, CVBestSubsetsResults, CVGroupPathResults, CVGroupResults, CVPathResults,
                       CVResults, BestGroupSubsetsBootstrapResults, BestGroupSubsetsResults, BestSubsetsBootstrapResults, BestSubsetsResults, BootstrapResults, InteractionBootstrapResults, InteractionResults, MultiGroupResults,
                       MultiResponseResults, OwenResults, PermutationTestResults,
                       SampledBootstrapGroupResults, SampledBootstrapResults, SampledCVGroupResults, SampledCVResults, SampledInteractionResults, SampledMultiGroupResults, SampledMultiResults, ShapleyResults, SizeIncompatible,
                       TopGroupSubsetsCVResults, TopGroupSubsetsResults, TopSubsetsCVResults, TopSubsetsResults,
                       validate_data)
from ._stats import error_estimates, error_estimates_lowrank, merge_sample_cov, merge_sample_mean
from ._driver import (ls_spa, ls_spa_cv, ls_spa_cv_path, ls_spa_cv_sampled, ls_spa_best_subsets_cv, cv_fold_ids, ls_spa_best_group_subsets_bootstrap, ls_spa_best_subsets, ls_spa_best_subsets_bootstrap, ls_spa_bootstrap, ls_spa_bootstrap_sampled, ls_spa_groups, ls_spa_interactions, ls_spa_interactions_bootstrap,
                      ls_spa_interactions_sampled, ls_spa_multi, ls_spa_multi_sampled, ls_spa_owen,
                      ls_spa_permutation_test, ls_spa_top_group_subsets, ls_spa_top_group_subsets_cv, ls_spa_top_subsets,
                      ls_spa_top_subsets_cv,
                      reduce_data, square_shapley, run_estimator, release)
from ._native import LSSPANativeError
from ._rccl import NativeComm

__all__ = [
    "ls_spa", "ls_spa_bootstrap", "BootstrapResults", "ls_spa_groups", "ls_spa_interactions", "ls_spa_interactions_sampled", "SampledInteractionResults",
    "ShapleyResults", "InteractionResults", "SizeIncompatible", "validate_data", "merge_sample_mean",
    "merge_sample_cov", "square_shapley", "reduce_data", "error_estimates",
    "error_estimates_lowrank", "run_estimator", "release", "LSSPANativeError", "NativeComm",
    "ls_spa_interactions_bootstrap", "InteractionBootstrapResults", "ls_spa_multi", "MultiResponseResults",
    "MultiGroupResults", "ls_spa_multi_sampled", "SampledMultiResults", "SampledMultiGroupResults",
    "ls_spa_permutation_test", "PermutationTestResults", "ls_spa_owen", "OwenResults",
    "ls_spa_best_subsets", "BestSubsetsResults", "BestGroupSubsetsResults",
    "ls_spa_best_subsets_bootstrap", "BestSubsetsBootstrapResults",
    "ls_spa_best_group_subsets_bootstrap", "BestGroupSubsetsBootstrapResults",
    "ls_spa_top_subsets", "TopSubsetsResults",
    "ls_spa_top_group_subsets", "TopGroupSubsetsResults",
    "ls_spa_cv", "CVResults", "ls_spa_best_subsets_cv", "CVBestSubsetsResults", "cv_fold_ids",
    "CVGroupResults", "CVBestGroupSubsetsResults",
    "ls_spa_top_subsets_cv", "TopSubsetsCVResults",
    "ls_spa_top_group_subsets_cv", "TopGroupSubsetsCVResults",
    "ls_spa_cv_path", "CVPathResults", "CVGroupPathResults",
    "ls_spa_cv_sampled", "SampledCVResults", "SampledCVGroupResults",
    "ls_spa_bootstrap_sampled", "SampledBootstrapResults", "SampledBootstrapGroupResults",
]
