"""Truth of the K-fold cross-validation calls over groups of columns (include/lsspa.h, lsspa_cv_groups_*)  --  TEST
INFRASTRUCTURE, NOT PRODUCT CODE.

The fold problems are tests/cv_ref.py's, formed in long double and rounded to fp64 once; on each of them the grouped
value function of tests/test_groups_host.py gives u_f(S) = v_f(baseline + columns of the groups in S) of every one of
the 2^g group masks (bit k = group k; one fp64 solve per mask, error ~1e-14).  From the table: the fold-order sum u_cv,
the Shapley value of the group game, and the best per size under the library's total order (tests/cv_ref.py's best, with
a per-mask `ok`).

The cases are the layouts of tests/group_best_ref.py's CASES as (group sizes, baseline columns, label shuffle), on one
data set of N_ROWS rows each -- every training fold has more rows than p at K = 2 already.  Seeds picked on the CPU so
that, in the CV values, winner and runner-up of every size are more than MIN_GAP apart for every K the GPU tests use
(tests/test_cv_groups_host.py asserts it)."""
import functools

import numpy as np

import cv_ref as R
import group_best_ref as GB
from test_groups_host import group_values, labels_of, shapley_of_table

MIN_GAP = GB.MIN_GAP
NAMES = ("gl0", "gl6", "mixed", "alllow", "nine")
KS = (2, 5)
N_ROWS = 120
# name -> seed of cv_ref.data(p, N_ROWS, seed)
SEEDS = {"gl0": 901, "gl6": 902, "mixed": 903, "alllow": 904, "nine": 905}
# beside NAMES x KS: "mixed" once at K = 32 on 400 rows
WIDE = ("mixed", 32, 400)
FOLD_SEED = 7

# The layout that runs in several launches and units (tests/test_gpu_cv_groups.py): low groups of 1, 1 and 3 columns
# (ql = 5: the next group of 3 no longer fits), fifteen high groups of 3 and a baseline of 14, p = 64; K = 2 on 300
# rows.  8192 units of per = 4; a subset's matrix has 43 rows on average, which leaves a launch 36295 high subsets, two
# steps of a unit at K = 2: two launches (tests/test_cv_groups_host.py asserts it from the plan function).
MULTI_SIZES, MULTI_NB, MULTI_K, MULTI_N, MULTI_SEED = [1, 1, 3] + [3] * 15, 14, 2, 300, 911


def multi_labels():
    return labels_of(MULTI_SIZES, MULTI_NB, seed=12)


def case_labels(name):
    sizes, nb, shuffle, _ = GB.CASES[name]
    return labels_of(sizes, nb, seed=shuffle)


def fold_values(X, y, ids, K, labels, reg=0.0, masks=None):
    """u_fold [len(masks)][K] (fp64): u_f of the group masks (all 2^g of them by default) on every fold problem."""
    g = int(np.max(labels)) + 1
    masks = np.arange(1 << g) if masks is None else np.asarray(masks)
    probs, yy = R.problems(X, y, ids, K, reg)
    cols = []
    for G, gv, H, h in probs:
        f64 = [np.asarray(a, dtype=np.float64) for a in (G, gv, H, h)]
        cols.append(group_values(*f64, float(yy), labels, masks))
    return np.stack(cols, axis=1)


def seq_sum(cols):
    """fp64 sum of the columns of cols [n][K] in ascending order, as the device forms it"""
    total = cols[:, 0].copy()
    for f in range(1, cols.shape[1]):
        total = total + cols[:, f]
    return total


def cv_values(X, y, ids, K, labels, reg=0.0, masks=None):
    """(u_cv [n], u_fold [n][K])"""
    uf = fold_values(X, y, ids, K, labels, reg, masks)
    return seq_sum(uf), uf


def shapley(u, g):
    """phi [g] of the group game with the table u [2^g]"""
    return shapley_of_table(np.asarray(u, dtype=np.float64), g)


def best(u, g, ok=None):
    """(best [g + 1], masks [g + 1], found [g + 1], runner [g + 1]) under the library's order: the larger value, on equal
    values the smaller mask; ok [2^g] bool: the candidates"""
    return R.best(np.asarray(u, dtype=np.float64), g, 0, ok)


@functools.lru_cache(maxsize=None)
def case(name, K, n=N_ROWS, reg=0.0):
    """(X, y, ids, labels, u_cv, u_fold) of a named case: computed once, shared by the tests, never written."""
    labels = case_labels(name)
    X, y = R.data(len(labels), n, seed=SEEDS[name])
    ids = R.fold_ids(n, K, seed=FOLD_SEED)
    u, uf = cv_values(X, y, ids, K, labels, reg)
    for a in (X, y, ids, labels, u, uf):
        a.setflags(write=False)
    return X, y, ids, labels, u, uf


def columns_of(labels, mask):
    return GB.columns_of(labels, mask)


def lstsq_value(X, y, ids, K, labels, mask):
    """The independent restatement (reg = 0): per fold, fit the selected columns on the other folds' rows with lstsq,
    predict the fold, and divide by the pooled ||y||^2.  (u_cv, [u_f])"""
    cols = np.nonzero(columns_of(labels, mask))[0]
    yy = float(y @ y)
    out = []
    for f in range(K):
        te = ids == f
        if len(cols) == 0:
            out.append(0.0)
            continue
        theta = np.linalg.lstsq(X[~te][:, cols], y[~te], rcond=None)[0]
        r = y[te] - X[te][:, cols] @ theta
        out.append(float(y[te] @ y[te] - r @ r) / yy)
    return sum(out), out


# ---- the exact-tie problem -------------------------------------------------------------------------------------------
# tests/group_best_ref.py's construction on one data set: groups a (one column), b and c (seven each) are nonzero only
# on rows whose y is 0, so every fold's g = X^T y / W is exactly 0 on their columns and u_f(S) = 0.0 exactly for every S
# within {a, b, c}, in any arithmetic and in every fold.  Groups d (one column) and e (two) carry the signal, with its
# sign flipped between the two folds: a model that holds one of them predicts the other fold with the wrong sign and is
# worse than 0.  The layout makes a, d, e low and b, c high.  Two numberings of the groups, as TIE_RUNS there.
TIE_SIZES, TIE_RUNS, tie_winners = GB.TIE_SIZES, GB.TIE_RUNS, GB.tie_winners


@functools.lru_cache(maxsize=None)
def tie_case(run):
    """(X, y, ids, labels, u_cv of all 32 masks) of the exact-tie problem under the run's numbering; K = 2."""
    rng = np.random.default_rng(78)
    n0, n1 = 60, 60                          # rows with y = 0 (both folds), rows with the signal (both folds)
    order = "abcde"
    width = [TIE_SIZES[k] for k in order]
    start = np.concatenate([[0], np.cumsum(width)])
    p = int(start[-1])
    X = np.zeros((n0 + n1, p))
    abc, sig = slice(0, int(start[3])), slice(int(start[3]), p)
    X[:n0, abc] = rng.integers(-3, 4, size=(n0, int(start[3]))).astype(float)
    X[n0:, sig] = rng.standard_normal((n1, 3))
    ids = (np.arange(n0 + n1) % 2).astype(np.int32)
    w = np.array([1.0, 0.8, -0.7])
    sign = np.where(ids[n0:] == 0, 1.0, -1.0)
    y = np.concatenate([np.zeros(n0), sign * (X[n0:, sig] @ w) + 0.1 * rng.standard_normal(n1)])
    labels = np.concatenate([np.full(TIE_SIZES[k], TIE_RUNS[run][k]) for k in order]).astype(np.int64)
    perm = rng.permutation(p)                # the columns in no particular order
    X, labels = X[:, perm], labels[perm]
    u, _ = cv_values(X, y, ids, 2, labels)
    for a in (X, y, ids, labels, u):
        a.setflags(write=False)
    return X, y, ids, labels, u
