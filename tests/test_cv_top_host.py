"""Top lists by the K-fold cross-validated R^2 -- CPU side: every refusal of ls_spa_top_subsets_cv (raised without
touching an engine), the plan of the list kernel against a restatement of its formula, the driver through a NumPy
double of the engine whose numbers are the truth of tests/cv_ref.py, the one-standard-error fields against the
restatement of tests/cv_top_ref.py, and the margins of the truth lists the GPU test compares masks with."""
import warnings

import numpy as np
import pytest

import cv_ref as R
import cv_top_ref as CT
from ls_spa import (SizeIncompatible, TopSubsetsCVResults, ls_spa_best_subsets_cv, ls_spa_top_subsets_cv)
from ls_spa._engine import debug_cv_plan, debug_cv_top_plan, debug_subsets_top_plan
from test_cv_host import CVOracleEngine, Untouchable


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_engine():
    X, y = R.data(5, 30, seed=4)
    eng = Untouchable()
    call = ls_spa_top_subsets_cv
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
    with pytest.raises(ValueError, match="identically zero"):
        call(X, np.zeros(30), _engine=eng)
    for bad in (0, 17, -1, 2.0, True, "3", None):
        with pytest.raises(ValueError, match="n_best must be an integer in 1 .. 16"):
            call(X, y, n_best=bad, _engine=eng)
    for bad in ([5], [-1], [1, 1], [0.5], "01"):
        with pytest.raises(ValueError, match="include"):
            call(X, y, include=bad, _engine=eng)
    with pytest.raises(TypeError):
        call(X, y, groups=[0, 0, 1, 1, 2], _engine=eng)       # the grouped call is not built


# ---- the plan ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p, K, T", [(6, 2, 1), (14, 3, 16), (20, 2, 4), (32, 32, 16)])
def test_plan(p, K, T):
    plan = debug_cv_top_plan(p, K, T)
    q = min(p, 6)
    n_high = 1 << (p - q)
    units = min(n_high, 8192)
    per = n_high // units
    steps = min(per, max(1, (1 << 20) // (units * K)))
    assert (plan["units"], plan["per"], plan["steps"], plan["launches"]) == (units, per, steps, -(-per // steps))
    cut = debug_cv_plan(p, K)                                 # the cut is cv_best's, the table subsets_top's
    assert all(plan[k] == cut[k] for k in ("units", "per", "steps", "launches", "workgroup"))
    lists = 20 * (12 * T + 4)                                 # 20 lists of T (value, mask) and a count
    assert plan["lds_bytes"] == cut["lds_bytes"] + lists and plan["workgroup"] == 64
    assert plan["lds_bytes"] <= 160 * 1024 // (7 if T == 1 else 6)      # workgroups a CU: seven at T = 1, six at 16
    assert plan["sizes"] == min(p, (per.bit_length() - 1) + q) + 1 <= 20
    assert plan["table_bytes"] == units * (p + 1) * (12 * T + 4)
    one = debug_subsets_top_plan(p, T)
    assert plan["sizes"] == one["sizes"] and plan["table_bytes"] == one["table_bytes"]


def test_plan_refusals():
    for p, K, T in [(0, 5, 4), (33, 5, 4), (8, 1, 4), (8, 33, 4), (8, 5, 0), (8, 5, 17)]:
        with pytest.raises(ValueError):
            debug_cv_top_plan(p, K, T)


# ---- the driver on a test double ---------------------------------------------------------------------------------------
class CVTopOracleEngine(CVOracleEngine):
    """CVOracleEngine with cv_top: the lists of tests/cv_top_ref.py over the double's own values.  table: per-fold values
    [2^p][K] that replace the truth after the load (a constructed game); drop: sizes it lists nothing for."""

    def __init__(self, info=None, drop=(), table=None):
        super().__init__(info, drop)
        self._table = table

    def cv_load(self, X, y, fold_ids, K, reg):
        super().cv_load(X, y, fold_ids, K, reg)
        if self._table is not None:
            self._vf = np.array(self._table, dtype=np.float64)
            self._v = self._vf[:, 0].copy()
            for f in range(1, K):
                self._v = self._v + self._vf[:, f]

    def cv_top(self, include=0, n_best=10, steps=0):
        self.calls.append(("top", include, n_best))
        v, masks, count = CT.top_lists(self._v, self._p, n_best, include)
        for k in self._drop:
            v[k], masks[k], count[k] = np.nan, 0, 0
        v_fold = np.full((self._p + 1, n_best, self._K), np.nan)
        for k in range(self._p + 1):
            v_fold[k, :count[k]] = self._vf[masks[k, :count[k]].astype(np.int64)]
        return v, masks, count, v_fold, self._bits()


def masks_of(subsets):
    return (subsets.astype(np.int64) << np.arange(subsets.shape[-1])).sum(axis=-1)


def check_one_se(res):
    b, gap, se, within, one = CT.one_se(res.sizes, res.n_models, res.r_squared, res.fold_r_squared)
    assert res.best_size == (int(res.sizes[b]) if b >= 0 else -1)
    np.testing.assert_array_equal(res.best_gap, gap)
    np.testing.assert_allclose(res.best_gap_std_error, se, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(res.within_one_se, within)
    assert res.one_se_size == (int(res.sizes[one]) if one >= 0 else -1)
    if one >= 0:
        np.testing.assert_array_equal(res.one_se_subset, res.subsets[one, 0])
        assert res.within_one_se[b, 0] and res.best_gap[b, 0] == 0.0 and res.best_gap_std_error[b, 0] == 0.0
        assert res.one_se_size <= res.best_size
    else:
        assert not res.one_se_subset.any()


@pytest.mark.parametrize("include", [None, [2, 5]])
def test_ls_spa_top_subsets_cv_on_the_double(include):
    p, K, n, T = 7, 3, 60, 5
    X, y = R.data(p, n, seed=8)
    inc = sum(1 << j for j in include or ())
    k0 = len(include or ())
    eng = CVTopOracleEngine()
    res = ls_spa_top_subsets_cv(X, y, 0.1, K, T, include=include, seed=3, _engine=eng)
    assert isinstance(res, TopSubsetsCVResults)
    assert eng.calls == [("load", K, 0.1), ("top", inc, T), ("free",)]
    ns = p + 1 - k0
    assert res.sizes.tolist() == list(range(k0, p + 1))
    assert res.subsets.shape == (ns, T, p) and res.r_squared.shape == (ns, T) and res.theta.shape == (ns, T, p)
    assert res.fold_r_squared.shape == (ns, T, K) and res.gap.shape == (ns, T)
    np.testing.assert_array_equal(res.fold_ids, R.fold_ids(n, K, seed=3))
    v, vf = R.cv_values(X, y, res.fold_ids, K, 0.1)
    want_v, want_m, want_c = CT.top_lists(v, p, T, inc)
    np.testing.assert_array_equal(res.n_models, want_c[k0:])
    from math import comb
    assert res.n_models.tolist() == [min(T, comb(p - k0, k - k0)) for k in res.sizes]
    listed = np.arange(T)[None, :] < res.n_models[:, None]
    np.testing.assert_array_equal(masks_of(res.subsets)[listed], want_m[k0:][listed])
    np.testing.assert_allclose(res.r_squared[listed], want_v[k0:][listed], rtol=0, atol=1e-14)
    assert np.isnan(res.r_squared[~listed]).all() and np.isnan(res.theta[~listed]).all()
    assert np.isnan(res.fold_r_squared[~listed]).all() and not res.subsets[~listed].any()
    assert np.isnan(res.gap[~listed]).all() and np.isnan(res.best_gap[~listed]).all()
    assert np.isnan(res.best_gap_std_error[~listed]).all() and not res.within_one_se[~listed].any()
    assert (res.subsets[listed].sum(axis=1) == np.broadcast_to(res.sizes[:, None], (ns, T))[listed]).all()
    if include:
        assert res.subsets[listed][:, include].all()
    assert (np.diff(res.r_squared, axis=1)[listed[:, 1:]] <= 0).all()
    np.testing.assert_allclose(res.fold_r_squared[listed].sum(axis=1), res.r_squared[listed], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(res.gap[listed], (res.r_squared[:, :1] - res.r_squared)[listed])
    # theta: the refit on ALL rows, exactly zero outside the subset
    G, g = X.T @ X / n + 0.1 * np.eye(p), X.T @ y / n
    for i, r in zip(*np.nonzero(listed)):
        cols = np.nonzero(res.subsets[i, r])[0]
        if len(cols):
            np.testing.assert_allclose(res.theta[i, r, cols], np.linalg.solve(G[np.ix_(cols, cols)], g[cols]), rtol=1e-11)
        assert (res.theta[i, r, ~res.subsets[i, r]] == 0.0).all()
    # the merge over sizes: the T best of everything listed, larger value then smaller mask
    flat_v, flat_m = res.r_squared[listed], masks_of(res.subsets)[listed]
    order = np.lexsort((flat_m, -flat_v))[:T]
    np.testing.assert_array_equal(res.top_r_squared, flat_v[order])
    np.testing.assert_array_equal(masks_of(res.top_subsets), flat_m[order])
    np.testing.assert_array_equal(res.top_sizes, res.top_subsets.sum(axis=1))
    assert res.top_r_squared[0] == np.nanmax(res.r_squared)
    # rank 0 is the selection's winner on the same double
    sel = ls_spa_best_subsets_cv(X, y, 0.1, K, include=include, seed=3, _engine=CVTopOracleEngine())
    np.testing.assert_array_equal(res.r_squared[:, 0], sel.r_squared)
    np.testing.assert_array_equal(res.subsets[:, 0], sel.subsets)
    np.testing.assert_array_equal(res.fold_r_squared[:, 0], sel.fold_r_squared)
    np.testing.assert_array_equal(res.theta[:, 0], sel.theta)
    assert res.best_size == sel.best_size and res.full_r_squared == sel.full_r_squared
    np.testing.assert_array_equal(res.best_subset, sel.best_subset)
    check_one_se(res)
    assert "cross-validation" in repr(res) and "one standard error" in repr(res)


def test_one_se_prefers_the_smaller_model():
    """A constructed game, p = 3, K = 4: the full model wins by 0.01 over {0}, but fold by fold the difference swings
    by +-0.03, so {0} is within one standard error; the models of size 2 lose every fold by the same 0.1 (standard error
    0) and the empty model loses by 0.81."""
    p, K = 3, 4
    table = np.zeros((8, K))
    table[0b001] = [0.20, 0.20, 0.20, 0.20]
    table[0b010] = table[0b100] = [0.02, 0.01, 0.02, 0.01]
    table[0b011] = [0.13, 0.07, 0.14, 0.07]
    table[0b101] = [0.12, 0.06, 0.13, 0.06]
    table[0b110] = [0.03, 0.02, 0.03, 0.02]
    table[0b111] = [0.23, 0.17, 0.24, 0.17]
    X, y = R.data(p, 24, seed=1)
    res = ls_spa_top_subsets_cv(X, y, folds=K, n_best=3, _engine=CVTopOracleEngine(table=table))
    assert res.best_size == 3 and res.one_se_size == 1 and res.one_se_subset.tolist() == [True, False, False]
    d = table[0b111] - table[0b001]
    assert res.best_gap[1, 0] == res.r_squared[3, 0] - res.r_squared[1, 0] and abs(res.best_gap[1, 0] - 0.01) < 1e-15
    assert abs(res.best_gap_std_error[1, 0] - 2.0 * np.std(d, ddof=1)) < 1e-15
    assert res.within_one_se[1, 0] and not res.within_one_se[1, 1:].any()
    assert not res.within_one_se[0].any() and res.within_one_se[3, 0]
    # {0, 1} loses every fold by the same 0.10: a gap the folds agree on, standard error (almost) zero
    assert abs(res.best_gap[2, 0] - 0.40) < 1e-15 and res.best_gap_std_error[2, 0] < 1e-15
    assert not res.within_one_se[2].any()
    check_one_se(res)


def test_warning_names_the_folds_and_empty_sizes():
    p, K, T = 5, 4, 3
    X, y = R.data(p, 40, seed=9)
    with pytest.warns(RuntimeWarning, match=r"fold\(s\) 1, 3 "):
        res = ls_spa_top_subsets_cv(X, y, folds=K, n_best=T, _engine=CVTopOracleEngine(info=[0, 1, 0, 1], drop=(2, 5)))
    assert res.n_models.tolist() == [1, 3, 0, 3, 3, 0]
    assert np.isnan(res.r_squared[[2, 5]]).all() and not res.subsets[[2, 5]].any()
    assert not res.within_one_se[[2, 5]].any() and res.best_size in (0, 1, 3, 4)
    check_one_se(res)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ls_spa_top_subsets_cv(X, y, folds=K, n_best=T, _engine=CVTopOracleEngine())
        res = ls_spa_top_subsets_cv(X, y, folds=K, n_best=T, _engine=CVTopOracleEngine(drop=range(p + 1)))
    assert res.best_size == -1 and res.one_se_size == -1 and not res.best_subset.any() and not res.one_se_subset.any()
    assert len(res.top_r_squared) == 0 and not res.within_one_se.any() and np.isnan(res.best_gap).all()


# ---- the margins of the GPU truth test's cases -------------------------------------------------------------------------
@pytest.mark.parametrize("p, K", sorted(CT.TRUTH_SEEDS))
def test_truth_lists_have_a_clear_margin(p, K):
    """Inside every size's top-17 of the long-double truth neighbours differ by more than 1e-9: the device's values are
    within 1e-11 of it, so its lists at every T <= 16 must hold the truth's masks in the truth's order."""
    _, _, _, v, _ = CT.truth_case(p, K)
    m = CT.margin(v, p, CT.T_MAX)
    print("p", p, "K", K, "seed", CT.TRUTH_SEEDS[(p, K)], "margin", m)
    assert m > 1e-9
