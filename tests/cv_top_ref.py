"""Truth of ls_spa_top_subsets_cv  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The T best subsets of every size by the K-fold cross-validated value: the long-double values of tests/cv_ref.py sorted by
tests/top_ref.top_truth (larger value, then smaller mask; bit j = feature j), the margins of such lists (what a test
needs to be far above the device's rounding before it compares masks), the shared cases of the GPU truth test, and the
one-standard-error statistics of the public call restated with plain loops.
"""
import functools
import math

import numpy as np

import cv_ref as R
import top_ref

T_MAX = top_ref.T_MAX

# (p, K) -> seed of the GPU truth test's case: chosen on the CPU (tests/test_cv_top_host.py asserts it for every entry)
# so that inside every size's top-(T_MAX + 1) list of the long-double truth neighbours differ by more than 1e-9
TRUTH_SEEDS = {(1, 2): 0, (6, 2): 0, (7, 2): 0, (12, 2): 0, (1, 5): 0, (6, 5): 0, (7, 5): 0, (12, 5): 0}


@functools.lru_cache(maxsize=None)
def case(p, K, n=120, seed=0, reg=0.0):
    """(X, y, ids, v [2^p], v_fold [2^p][K]): data of cv_ref.data(p, n, 100 p + seed), the folds of seed 7 and, for
    p <= 12, the long-double truth.  Computed once, shared, never written."""
    X, y = R.data(p, n, seed=100 * p + seed)
    ids = R.fold_ids(n, K, seed=7)
    v, vf = R.cv_values(X, y, ids, K, reg) if p <= 12 else (None, None)
    for a in (X, y, ids, v, vf):
        if a is not None:
            a.setflags(write=False)
    return X, y, ids, v, vf


def truth_case(p, K):
    return case(p, K, seed=TRUTH_SEEDS[(p, K)])


def top_lists(v_all, p, T, include=0, valid=None):
    """(v [p + 1][T] float64, masks [p + 1][T] uint32, count [p + 1]) of a table of all 2^p values: top_ref.top_truth."""
    return top_ref.top_truth(np.asarray(v_all).astype(np.float64), p, T, include, valid)


def margin(v_all, p, T):
    """The smallest difference between neighbours inside any size's T + 1 best values of the table v_all (long double):
    adjacent entries of the top-T list, and its last entry against the first one left out.  inf if no size has two."""
    v_all = np.asarray(v_all)
    size = np.array([bin(m).count("1") for m in range(1 << p)])
    worst = math.inf
    for k in range(p + 1):
        vals = np.sort(v_all[size == k])[::-1][:T + 1]
        if len(vals) > 1:
            worst = min(worst, float((vals[:-1] - vals[1:]).min()))
    return worst


def one_se(sizes, n_models, r_squared, fold_r_squared):
    """(best_row, best_gap [n][T], std_error [n][T], within [n][T], one_se_row): the statistics of the public call by
    plain loops.  b = rank 0 of the first row with the largest rank-0 value; for a listed model d_f = fold[b][f] -
    fold[i, r][f], gap = r2[b] - r2[i, r], se = sqrt(K) sqrt(sum (d_f - mean d)^2 / (K - 1)); within = gap <= se; one_se_row
    the first row whose rank 0 is within.  -1 / NaN / False where nothing is listed."""
    n, T, K = fold_r_squared.shape
    gap, se = np.full((n, T), np.nan), np.full((n, T), np.nan)
    within = np.zeros((n, T), dtype=bool)
    b = -1
    for i in range(n):
        if n_models[i] > 0 and (b < 0 or r_squared[i, 0] > r_squared[b, 0]):
            b = i
    if b < 0:
        return -1, gap, se, within, -1
    for i in range(n):
        for r in range(int(n_models[i])):
            d = [float(fold_r_squared[b, 0, f]) - float(fold_r_squared[i, r, f]) for f in range(K)]
            mean = math.fsum(d) / K
            var = math.fsum((x - mean) ** 2 for x in d) / (K - 1)
            gap[i, r] = float(r_squared[b, 0]) - float(r_squared[i, r])
            se[i, r] = math.sqrt(K) * math.sqrt(var)
            within[i, r] = gap[i, r] <= se[i, r]
    one = next(i for i in range(n) if n_models[i] > 0 and within[i, 0])
    return b, gap, se, within, one
