"""Truth of the sampled K-fold CV attribution (ls_spa_cv_sampled, lsspa_cv_lift_* of include/lsspa.h), by tests/hp_ref.py.

Fold problem f is hp_ref.Problem(X[ids != f], X[ids == f], y[ids != f], y[ids == f], reg): trained on the other folds'
rows, tested on fold f.  A Problem's lifts divide by its own ||y_f||^2; the game divides every fold by the pooled
||y||^2, so fold f's lifts are scaled by yy_f / yy_pooled in long double and a sample's lift vector is their sum over the
folds in long double.  plain_*: the same with hp_ref.plain_lifts (NumPy / LAPACK in fp64), the yardstick of the
tolerance rule."""
import numpy as np

import hp_ref


def fold_problems(X, y, ids, K, reg=0.0):
    """([K] hp_ref.Problem, scale [K] long double: yy_f / yy_pooled)"""
    X, y, ids = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(ids)
    probs = [hp_ref.Problem(X[ids != f], X[ids == f], y[ids != f], y[ids == f], reg) for f in range(K)]
    yl = np.asarray(y, dtype=np.longdouble)
    yy = np.array([(yl[ids == f] * yl[ids == f]).sum() for f in range(K)], dtype=np.longdouble)
    return probs, yy / yy.sum()


def truth_lifts(probs, scale, orders, antithetical):
    """(fold [B][K][p], total [B][p]) as fp64 roundings of the long-double values"""
    fold = np.array([[p.lifts([o], antithetical, raw=True)[0] * s for p, s in zip(probs, scale)] for o in orders],
                    dtype=np.longdouble)
    return np.asarray(fold, dtype=np.float64), np.asarray(fold.sum(axis=1), dtype=np.float64)


def plain_lifts(X, y, ids, K, reg, orders, antithetical):
    """The plain restatement: (fold [B][K][p], total [B][p]) by hp_ref.plain_lifts per fold, scaled and summed in fp64
    long double like the truth."""
    X, y, ids = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(ids)
    yl = np.asarray(y, dtype=np.longdouble)
    yy = np.array([(yl[ids == f] * yl[ids == f]).sum() for f in range(K)], dtype=np.longdouble)
    scale = yy / yy.sum()
    per = [hp_ref.plain_lifts(X[ids != f], X[ids == f], y[ids != f], y[ids == f], reg, orders, antithetical)
           for f in range(K)]
    fold = np.stack([np.asarray(per[f], dtype=np.longdouble) * scale[f] for f in range(K)], axis=1)
    return np.asarray(fold, dtype=np.float64), np.asarray(fold.sum(axis=1), dtype=np.float64)


def group_fold(lifts, labels):
    """[..., g] from column lifts [..., p]: group k's columns added in ascending column order from 0.0 (the device's)."""
    labels = np.asarray(labels)
    g = int(labels.max()) + 1
    out = np.zeros(lifts.shape[:-1] + (g,), dtype=lifts.dtype)
    for k in range(g):
        acc = np.zeros(lifts.shape[:-1], dtype=lifts.dtype)
        for c in np.nonzero(labels == k)[0]:
            acc = acc + lifts[..., c]
        out[..., k] = acc
    return out


def cv_value(probs, scale, cols):
    """v_cv(S) = sum_f scale_f v_f(S) in long double"""
    return sum(p.subset_value(cols) * s for p, s in zip(probs, scale))


def brute_shapley(probs, scale, p):
    """The Shapley value of the CV game over the p columns from the table of all subsets (p <= 10), long double."""
    from math import factorial
    vals = [cv_value(probs, scale, [j for j in range(p) if (m >> j) & 1]) for m in range(1 << p)]
    phi = np.zeros(p, dtype=np.longdouble)
    for j in range(p):
        for m in range(1 << p):
            if (m >> j) & 1:
                continue
            k = bin(m).count("1")
            w = np.longdouble(factorial(k) * factorial(p - 1 - k)) / np.longdouble(factorial(p))
            phi[j] += w * (vals[m | (1 << j)] - vals[m])
    return phi
