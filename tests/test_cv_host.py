"""K-fold cross-validation -- CPU side: the truth of tests/cv_ref.py vetted against the split formula and the linearity
of the Shapley value, the fold assignment, every refusal (raised without touching an engine), the plan of the selection
kernel, and the drivers through a NumPy double of the engine whose numbers are that truth."""
import warnings

import numpy as np
import pytest

import cv_ref as R
import perm_ref
from ls_spa import (CVBestSubsetsResults, CVResults, SizeIncompatible, cv_fold_ids, ls_spa_best_subsets_cv, ls_spa_cv)
from ls_spa._engine import debug_cv_plan, debug_subsets_top_plan


# ---- the truth ---------------------------------------------------------------------------------------------------------
def test_truth_sums_and_linearity():
    p, K, n = 6, 3, 60
    X, y = R.data(p, n, seed=1)
    ids = R.fold_ids(n, K, seed=2)
    v, vf = R.cv_values(X, y, ids, K, reg=0.1)
    phi = R.shapley(v, p)
    assert abs(float(phi.sum() - v[-1])) < 1e-17 and v[0] == 0
    per_fold = sum(R.shapley(vf[:, f], p) for f in range(K))
    assert np.abs((phi - per_fold).astype(np.float64)).max() < 1e-17
    # the CV value is the pooled out-of-sample R^2: 1 - sum_f ||y_f - X_f theta^(-f)||^2 / ||y||^2
    yy = np.asarray(y, dtype=R.LD) @ np.asarray(y, dtype=R.LD)
    cols = [0, 2, 5]
    want = sum(R.split_value(X[ids != f], X[ids == f], y[ids != f], y[ids == f], cols, yy, reg=0.1) for f in range(K))
    assert abs(float(v[0b100101] - want)) < 1e-12


def test_truth_two_folds_of_duplicated_data_equal_the_split_formula():
    p, n = 4, 40
    X, y = R.data(p, n, seed=3)
    X2, y2 = np.concatenate([X, X]), np.concatenate([y, y])
    ids = np.repeat([0, 1], n).astype(np.int32)
    v, vf = R.cv_values(X2, y2, ids, 2)
    yy = 2 * (np.asarray(y, dtype=R.LD) @ np.asarray(y, dtype=R.LD))
    for mask in (0b0001, 0b1010, 0b1111):
        cols = [j for j in range(p) if (mask >> j) & 1]
        one = R.split_value(X, X, y, y, cols, yy)
        assert abs(float(vf[mask, 0] - one)) < 1e-12 and abs(float(v[mask] - 2 * one)) < 1e-12


def test_truth_best_tie_rule():
    v = np.array([0.0, 0.5, 0.5, 0.2, 0.5, 0.7, 0.7, 0.1])          # p = 3
    best, masks, found, runner = R.best(v, 3)
    assert list(masks) == [0, 1, 5, 7] and list(best) == [0.0, 0.5, 0.7, 0.1] and runner[1] == 0.5
    best, masks, found, _ = R.best(v, 3, include=0b010, ok=np.arange(8) != 6)
    assert list(found) == [False, True, True, True] and list(masks) == [0, 2, 3, 7] and np.isnan(best[0])


# ---- the fold assignment ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, K", [(10, 2), (23, 5), (64, 32), (101, 7)])
def test_fold_assignment(n, K):
    ids, k = cv_fold_ids(n, K, seed=9)
    assert k == K and ids.dtype == np.int32
    np.testing.assert_array_equal(ids, R.fold_ids(n, K, seed=9))
    np.testing.assert_array_equal(ids, cv_fold_ids(n, K, seed=9)[0])             # a pure function of (seed, N, K)
    counts = np.bincount(ids, minlength=K)
    assert counts.max() - counts.min() <= 1 and counts.min() >= 1
    pi = perm_ref.indices(9, 0, 0, n)
    np.testing.assert_array_equal(ids[pi], np.arange(n) % K)
    np.testing.assert_array_equal(cv_fold_ids(n, K, shuffle=False)[0], np.arange(n) % K)
    assert (cv_fold_ids(n, K, seed=10)[0] != ids).any()
    given = (np.arange(n) * 3 % K)
    got, k = cv_fold_ids(n, given)
    np.testing.assert_array_equal(got, given)
    assert k == K


# ---- refusals ----------------------------------------------------------------------------------------------------------
class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched ({name}) before the arguments were checked")


@pytest.mark.parametrize("call", [ls_spa_cv, ls_spa_best_subsets_cv])
def test_refusals_come_before_any_engine(call):
    X, y = R.data(5, 30, seed=4)
    eng = Untouchable()
    with pytest.raises(SizeIncompatible):
        call(X, y[:-1], _engine=eng)
    with pytest.raises(ValueError, match="one-dimensional"):
        call(X, y[:, None], _engine=eng)
    with pytest.raises(ValueError, match="at most p = 32"):
        call(np.ones((40, 33)), np.ones(40), _engine=eng)
    for K in (1, 33, 0):
        with pytest.raises(ValueError, match="2 .. 32 folds"):
            call(X, y, folds=K, _engine=eng)
    with pytest.raises(ValueError, match="integer"):
        call(X, y, folds=2.5, _engine=eng)
    with pytest.raises(ValueError, match="empty"):
        call(X[:3], y[:3], folds=4, _engine=eng)
    labels = np.arange(30) % 3
    with pytest.raises(ValueError, match="0 .. K-1"):
        call(X, y, folds=np.where(labels == 0, -1, labels), _engine=eng)
    with pytest.raises(ValueError, match="fold 1 of 3 is empty"):
        call(X, y, folds=np.where(labels == 1, 0, labels), _engine=eng)
    with pytest.raises(ValueError, match="shape"):
        call(X, y, folds=labels[:-1], _engine=eng)
    with pytest.raises(ValueError, match="integers"):
        call(X, y, folds=labels + 0.5, _engine=eng)
    with pytest.raises(ValueError, match="identically zero"):
        call(X, np.zeros(30), _engine=eng)


def test_include_refusals_come_before_any_engine():
    X, y = R.data(5, 30, seed=4)
    for bad in ([5], [-1], [1, 1], [0.5], "01"):
        with pytest.raises(ValueError, match="include"):
            ls_spa_best_subsets_cv(X, y, include=bad, _engine=Untouchable())


# ---- the plan ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 5, 32])
@pytest.mark.parametrize("p", [1, 6, 7, 14, 19, 20, 24, 32])
def test_plan(p, K):
    plan = debug_cv_plan(p, K)
    one = debug_subsets_top_plan(p, 1)                       # the one-problem enumeration's cut
    assert plan["units"] == one["units"] == min(1 << max(p - 6, 0), 8192) and plan["per"] == one["per"]
    assert plan["units"] * plan["per"] == 1 << max(p - 6, 0) and plan["per"] <= 1 << 13
    assert (plan["per"] > 1) == (p >= 20)
    assert 1 <= plan["steps"] <= plan["per"]
    assert plan["steps"] == min(plan["per"], max(1, (1 << 20) // (plan["units"] * K)))
    assert plan["launches"] == -(-plan["per"] // plan["steps"])
    assert plan["workgroup"] == 64 and 20000 < plan["lds_bytes"] <= 160 * 1024 // 7     # seven workgroups a CU


def test_plan_refusals():
    for p, K in [(0, 5), (33, 5), (8, 1), (8, 33)]:
        with pytest.raises(ValueError):
            debug_cv_plan(p, K)


# ---- the drivers on a test double --------------------------------------------------------------------------------------
class CVOracleEngine:
    """What the cross-validation drivers ask of an engine, computed by tests/cv_ref.py (rounded to fp64).  info: the
    folds' info words it reports; drop: sizes it reports as not found."""
    precision = "float64"
    p = 0

    def __init__(self, info=None, drop=()):
        self.calls, self._info, self._drop = [], info, tuple(drop)

    def cv_load(self, X, y, fold_ids, K, reg):
        self.calls.append(("load", K, reg))
        self._p, self._K = X.shape[1], K
        v, vf = R.cv_values(X, y, np.asarray(fold_ids), K, reg)
        self._vf = vf.astype(np.float64)
        self._v = self._vf[:, 0].copy()
        for f in range(1, K):
            self._v = self._v + self._vf[:, f]

    def cv_free(self):
        self.calls.append(("free",))

    def _bits(self):
        return np.zeros(self._K, dtype=np.int32) if self._info is None else np.asarray(self._info, dtype=np.int32)

    def cv_shapley(self):
        self.calls.append(("shapley",))
        fold = np.array([R.shapley(self._vf[:, f].astype(R.LD), self._p).astype(np.float64) for f in range(self._K)])
        phi = fold[0].copy()
        for f in range(1, self._K):
            phi = phi + fold[f]
        return phi, fold, self._vf[-1].copy(), self._bits()

    def cv_best(self, include=0, steps=0):
        self.calls.append(("best", include))
        best, masks, found, _ = R.best(self._v, self._p, include)
        v_fold = np.full((self._p + 1, self._K), np.nan)
        for k in self._drop:
            best[k], masks[k], found[k] = np.nan, 0, False
        v_fold[found] = self._vf[masks[found].astype(np.int64)]
        return best, masks, found, v_fold, self._bits()

    def debug_cv_values(self, masks, folds=True):
        m = np.asarray(masks).astype(np.int64)
        return self._v[m], (self._vf[m] if folds else None)

    def set_flags(self, flags):
        pass


def test_ls_spa_cv_on_the_double():
    p, K, n = 6, 4, 50
    X, y = R.data(p, n, seed=6)
    eng = CVOracleEngine()
    res = ls_spa_cv(X, y, 0.2, K, seed=3, _engine=eng)
    assert isinstance(res, CVResults) and eng.calls == [("load", K, 0.2), ("shapley",), ("free",)]
    ids = R.fold_ids(n, K, seed=3)
    np.testing.assert_array_equal(res.fold_ids, ids)
    v, vf = R.cv_values(X, y, ids, K, 0.2)
    np.testing.assert_allclose(res.attribution, R.shapley(v, p).astype(np.float64), rtol=0, atol=1e-14)
    assert res.fold_attribution.shape == (K, p) and res.fold_r_squared.shape == (K,)
    assert abs(res.attribution.sum() - res.r_squared) < 1e-13 and abs(res.r_squared - float(v[-1])) < 1e-14
    assert abs(res.fold_r_squared.sum() - res.r_squared) < 1e-15
    G = X.T @ X / n + 0.2 * np.eye(p)
    np.testing.assert_allclose(res.theta, np.linalg.solve(G, X.T @ y / n), rtol=1e-12)
    assert "cross-validation" in repr(res)
    same = ls_spa_cv(X, y, 0.2, ids, _engine=CVOracleEngine())          # the labels taken as given
    np.testing.assert_array_equal(same.attribution, res.attribution)
    other = ls_spa_cv(X, y, 0.2, K, shuffle=False, _engine=CVOracleEngine())
    np.testing.assert_array_equal(other.fold_ids, np.arange(n) % K)


def test_ls_spa_best_subsets_cv_on_the_double():
    p, K, n = 7, 3, 60
    X, y = R.data(p, n, seed=8)
    eng = CVOracleEngine()
    res = ls_spa_best_subsets_cv(X, y, folds=K, include=[2, 5], _engine=eng)
    assert isinstance(res, CVBestSubsetsResults) and eng.calls[1] == ("best", 0b100100) and eng.calls[-1] == ("free",)
    assert res.sizes.tolist() == list(range(2, p + 1)) and res.subsets.shape == (p - 1, p)
    assert res.fold_r_squared.shape == (p - 1, K) and res.theta.shape == (p - 1, p)
    assert res.subsets[:, [2, 5]].all() and res.subsets.sum(axis=1).tolist() == res.sizes.tolist()
    v, _ = R.cv_values(X, y, res.fold_ids, K)
    best, masks, found, _ = R.best(v, p, include=0b100100)
    np.testing.assert_allclose(res.r_squared, best[2:].astype(np.float64), rtol=0, atol=1e-14)
    np.testing.assert_allclose(res.fold_r_squared.sum(axis=1), res.r_squared, rtol=0, atol=1e-15)
    G, g = X.T @ X / n, X.T @ y / n
    for i in range(len(res.sizes)):
        cols = np.nonzero(res.subsets[i])[0]
        assert sum(1 << int(j) for j in cols) == masks[res.sizes[i]]
        np.testing.assert_allclose(res.theta[i, cols], np.linalg.solve(G[np.ix_(cols, cols)], g[cols]), rtol=1e-12)
        assert (res.theta[i, ~res.subsets[i]] == 0.0).all()
    assert res.best_size == int(res.sizes[np.argmax(res.r_squared)])
    np.testing.assert_array_equal(res.best_subset, res.subsets[res.best_size - 2])
    assert abs(res.full_r_squared - float(v[-1])) < 1e-14 and "Best model" in repr(res)


def test_warning_names_the_folds_and_nan_rows():
    p, K = 5, 4
    X, y = R.data(p, 40, seed=9)
    with pytest.warns(RuntimeWarning, match=r"fold\(s\) 1, 3 "):
        res = ls_spa_best_subsets_cv(X, y, folds=K, _engine=CVOracleEngine(info=[0, 1, 0, 1], drop=(2, 5)))
    assert np.isnan(res.r_squared[[2, 5]]).all() and np.isnan(res.theta[[2, 5]]).all()
    assert not res.subsets[[2, 5]].any() and np.isnan(res.fold_r_squared[[2, 5]]).all()
    assert res.best_size in (0, 1, 3, 4) and not np.isnan(res.r_squared[[0, 1, 3, 4]]).any()
    with pytest.warns(RuntimeWarning, match=r"fold\(s\) 0 "):
        ls_spa_cv(X, y, folds=K, _engine=CVOracleEngine(info=[1, 0, 0, 0]))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ls_spa_cv(X, y, folds=K, _engine=CVOracleEngine())
    eng = CVOracleEngine(drop=range(p + 1))
    res = ls_spa_best_subsets_cv(X, y, folds=K, _engine=eng)
    assert res.best_size == -1 and not res.best_subset.any()
