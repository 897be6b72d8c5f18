"""Top lists by the K-fold cross-validated R^2 over groups of columns -- CPU side: every refusal of
ls_spa_top_group_subsets_cv (raised without touching an engine), the plan of the list kernel, the driver through a
NumPy double of the engine whose numbers are the truth of tests/cv_groups_ref.py (every result field against plain-loop
restatements), and the margins of the truth lists the GPU test compares masks with."""
import warnings
from math import comb

import numpy as np
import pytest

import cv_groups_ref as CG
import cv_groups_top_ref as GT
import cv_ref as R
import ls_spa
from ls_spa import (SizeIncompatible, TopGroupSubsetsCVResults, TopSubsetsCVResults, ls_spa_best_subsets_cv,
                    ls_spa_top_group_subsets_cv, ls_spa_top_subsets_cv)
from ls_spa._engine import debug_cv_groups_plan, debug_cv_groups_top_plan
from test_cv_groups_host import CVGroupsOracleEngine, Untouchable


def test_exported():
    assert "ls_spa_top_group_subsets_cv" in ls_spa.__all__ and "TopGroupSubsetsCVResults" in ls_spa.__all__
    assert ls_spa.TopGroupSubsetsCVResults is TopGroupSubsetsCVResults


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_engine():
    X, y = R.data(6, 30, seed=4)
    eng = Untouchable()
    call = ls_spa_top_group_subsets_cv
    groups = np.array([-1, 0, 0, 1, 2, 2])
    with pytest.raises(TypeError, match="include"):                  # no such keyword: the baseline is the include set
        call(X, y, include=[0], groups=groups, _engine=eng)
    with pytest.raises(TypeError, match="groups"):                   # and the column call has no groups=
        ls_spa_top_subsets_cv(X, y, groups=groups, _engine=eng)
    # bad labels: the label errors of ls_spa(groups=)
    with pytest.raises(ValueError, match="one label per column"):
        call(X, y, groups=groups[:-1], _engine=eng)
    with pytest.raises(ValueError, match="integer labels"):
        call(X, y, groups=groups + 0.5, _engine=eng)
    with pytest.raises(ValueError, match="below -1"):
        call(X, y, groups=np.array([-2, 0, 0, 1, 2, 2]), _engine=eng)
    with pytest.raises(ValueError, match="no group at all"):
        call(X, y, groups=np.full(6, -1), _engine=eng)
    with pytest.raises(ValueError, match="gap in its numbering"):
        call(X, y, groups=np.array([-1, 0, 0, 3, 2, 2]), _engine=eng)
    with pytest.raises(ValueError, match="at most p = 64"):
        call(np.ones((80, 65)), np.ones(80), groups=np.arange(65) % 4, _engine=eng)
    with pytest.raises(ValueError, match="at most g = 32"):
        call(np.ones((80, 40)) + np.eye(80, 40), np.arange(80.0), groups=np.arange(40), _engine=eng)
    with pytest.raises(ValueError, match="at most p = 32"):          # the column call keeps its column limit
        ls_spa_top_subsets_cv(np.ones((40, 33)), np.ones(40), _engine=eng)
    for bad in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match="n_best must be an integer in 1 .. 16"):
            call(X, y, n_best=bad, groups=groups, _engine=eng)
    # the refusals of ls_spa_cv
    with pytest.raises(SizeIncompatible):
        call(X, y[:-1], groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="one-dimensional"):
        call(X, y[:, None], groups=groups, _engine=eng)
    for K in (1, 33, 0):
        with pytest.raises(ValueError, match="2 .. 32 folds"):
            call(X, y, folds=K, groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="integer"):
        call(X, y, folds=2.5, groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="empty"):
        call(X[:3], y[:3], folds=4, groups=groups, _engine=eng)
    ids = np.arange(30) % 3
    with pytest.raises(ValueError, match="0 .. K-1"):
        call(X, y, folds=np.where(ids == 0, -1, ids), groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="fold 1 of 3 is empty"):
        call(X, y, folds=np.where(ids == 1, 0, ids), groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="identically zero"):
        call(X, np.zeros(30), groups=groups, _engine=eng)


# ---- the plan ----------------------------------------------------------------------------------------------------------
def test_plan_of_the_multi_launch_case():
    plan = debug_cv_groups_top_plan(CG.multi_labels(), 2, 4)
    print(plan)
    assert plan["units"] == 8192 and plan["per"] == 4 and plan["steps"] == 2 and plan["launches"] == 2
    assert plan["sizes"] == 6
    cut = debug_cv_groups_plan(CG.multi_labels(), 2)
    for key in ("gl", "gh", "ql", "nb", "units", "per", "steps", "launches"):
        assert plan[key] == cut[key], key


@pytest.mark.parametrize("K, T", [(2, 1), (5, 4), (32, 16)])
@pytest.mark.parametrize("name", CG.NAMES + ("multi", "p64"))
def test_plan(name, K, T):
    labels = {"multi": CG.multi_labels(), "p64": np.arange(64) % 32}.get(name)
    labels = CG.case_labels(name) if labels is None else labels
    g = int(labels.max()) + 1
    plan, cut = debug_cv_groups_top_plan(labels, K, T), debug_cv_groups_plan(labels, K)
    for key in ("gl", "gh", "ql", "nb", "units", "per", "steps", "launches"):
        assert plan[key] == cut[key], key
    assert plan["workgroup"] == 256
    # the lists take 25 x 16 x 12 bytes, 25 counts and the ids: less than 5.1 KB beside the one-problem workgroup's
    # 43.6 KB, whatever K and T -- three workgroups in a CU's 160 KB where the selection kernel has two
    assert 43624 + 25 * (16 * 12 + 4) <= plan["lds_bytes"] <= 43624 + 5100
    assert 3 * plan["lds_bytes"] <= 160 * 1024 < 3 * cut["lds_bytes"]
    assert plan["lds_bytes"] == debug_cv_groups_top_plan(labels, 2, 16)["lds_bytes"]
    assert plan["sizes"] == min(g, (plan["per"].bit_length() - 1) + plan["gl"]) + 1 <= 25
    assert plan["table_bytes"] == plan["units"] * (g + 1) * (12 * T + 4)


def test_plan_refusals():
    ok = np.arange(6) % 3
    for K, T in [(1, 4), (33, 4), (0, 4), (5, 0), (5, 17), (5, -1)]:
        with pytest.raises(ValueError):
            debug_cv_groups_top_plan(ok, K, T)
    for bad in (np.array([0, 2, 2]), np.array([-1, -1]), np.arange(33), np.zeros(65, dtype=int), np.array([-2, 0])):
        with pytest.raises(ValueError):
            debug_cv_groups_top_plan(bad, 5, 4)


# ---- the driver on a test double ---------------------------------------------------------------------------------------
class CVGroupsTopOracleEngine(CVGroupsOracleEngine):
    """CVGroupsOracleEngine with cv_groups_top: the lists of tests/cv_groups_top_ref.py over the double's own values.
    table: per-fold values [2^g][K] that replace the truth (a constructed game); drop: sizes it lists nothing for."""

    def __init__(self, info=None, drop=(), table=None):
        super().__init__(info, drop)
        self._fixed = table

    def _table(self, labels):
        if self._fixed is None:
            return super()._table(labels)
        uf = np.array(self._fixed, dtype=np.float64)
        return CG.seq_sum(uf), uf, int(np.max(labels)) + 1

    def cv_groups_top(self, labels, n_best=10, steps=0):
        self.calls.append(("top", n_best))
        u_all, uf, g = self._table(labels)
        u, masks, count = GT.top_lists(u_all, g, n_best)
        for k in self._drop:
            u[k], masks[k], count[k] = np.nan, 0, 0
        u_fold = np.full((g + 1, n_best, self._K), np.nan)
        for k in range(g + 1):
            u_fold[k, :count[k]] = uf[masks[k, :count[k]].astype(np.int64)]
        return u, masks, count, u_fold, self._bits()


def check_one_se(res):
    b, gap, se, within, one = GT.one_se(res.sizes, res.n_models, res.r_squared, res.fold_r_squared)
    assert res.best_size == (int(res.sizes[b]) if b >= 0 else -1)
    np.testing.assert_array_equal(res.best_gap, gap)
    np.testing.assert_allclose(res.best_gap_std_error, se, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(res.within_one_se, within)
    assert res.one_se_size == (int(res.sizes[one]) if one >= 0 else -1)
    if one >= 0:
        np.testing.assert_array_equal(res.one_se_group_subset, res.group_subsets[one, 0])
        np.testing.assert_array_equal(res.one_se_subset, res.subsets[one, 0])
        assert res.within_one_se[b, 0] and res.best_gap[b, 0] == 0.0 and res.best_gap_std_error[b, 0] == 0.0
        assert res.one_se_size <= res.best_size
    else:
        assert not res.one_se_subset.any() and not res.one_se_group_subset.any()


def test_ls_spa_top_group_subsets_cv_on_the_double():
    K, T, reg = 5, 6, 0.1
    X, y, ids, labels, _, _ = CG.case("nine", K)
    g, n, p = GT.n_groups(labels), len(y), len(labels)
    eng = CVGroupsTopOracleEngine()
    res = ls_spa_top_group_subsets_cv(X, y, labels, reg, ids, T, _engine=eng)
    assert isinstance(res, TopGroupSubsetsCVResults)
    assert eng.calls == [("load", K, reg), ("top", T), ("free",)]
    assert res.sizes.tolist() == list(range(g + 1))
    assert res.group_subsets.shape == (g + 1, T, g) and res.subsets.shape == res.theta.shape == (g + 1, T, p)
    assert res.r_squared.shape == res.gap.shape == res.n_columns.shape == (g + 1, T)
    assert res.fold_r_squared.shape == (g + 1, T, K)
    np.testing.assert_array_equal(res.fold_ids, ids)
    u, uf = CG.cv_values(X, y, ids, K, labels, reg)
    want_u, want_m, want_c = GT.top_lists(u, g, T)
    np.testing.assert_array_equal(res.n_models, want_c)
    assert res.n_models.tolist() == [min(T, comb(g, k)) for k in range(g + 1)]
    listed = np.arange(T)[None, :] < res.n_models[:, None]
    np.testing.assert_array_equal(GT.masks_of(res.group_subsets)[listed], want_m[listed])
    np.testing.assert_array_equal(res.r_squared[listed], want_u[listed])
    np.testing.assert_array_equal(res.fold_r_squared[listed], uf[want_m[listed].astype(np.int64)])
    np.testing.assert_array_equal(res.r_squared[listed], CG.seq_sum(res.fold_r_squared[listed]))
    # NaN / False / 0 past n_models
    assert (~listed).any()
    assert np.isnan(res.r_squared[~listed]).all() and np.isnan(res.theta[~listed]).all()
    assert np.isnan(res.fold_r_squared[~listed]).all() and np.isnan(res.gap[~listed]).all()
    assert not res.subsets[~listed].any() and not res.group_subsets[~listed].any()
    assert (res.n_columns[~listed] == 0).all() and np.isnan(res.best_gap[~listed]).all()
    assert np.isnan(res.best_gap_std_error[~listed]).all() and not res.within_one_se[~listed].any()
    # sizes, columns, coefficients: by plain loops
    G, gv = X.T @ X / n + reg * np.eye(p), X.T @ y / n
    for i, r in zip(*np.nonzero(listed)):
        assert int(res.group_subsets[i, r].sum()) == i
        want_cols = GT.columns_of(labels, res.group_subsets[i, r])
        np.testing.assert_array_equal(res.subsets[i, r], want_cols)
        np.testing.assert_array_equal(res.subsets[i, r], CG.columns_of(labels, int(want_m[i, r])))
        assert res.n_columns[i, r] == int(want_cols.sum())
        cols = np.nonzero(want_cols)[0]
        np.testing.assert_allclose(res.theta[i, r, cols], np.linalg.solve(G[np.ix_(cols, cols)], gv[cols]), rtol=1e-11)
        assert (res.theta[i, r, ~want_cols] == 0.0).all()
        assert res.gap[i, r] == res.r_squared[i, 0] - res.r_squared[i, r]
        if r:
            assert res.r_squared[i, r] <= res.r_squared[i, r - 1]
    # the merge over sizes: the T best of everything listed, larger value then smaller mask
    flat_v, flat_m = res.r_squared[listed], GT.masks_of(res.group_subsets)[listed]
    order = np.lexsort((flat_m, -flat_v))[:T]
    np.testing.assert_array_equal(res.top_r_squared, flat_v[order])
    np.testing.assert_array_equal(GT.masks_of(res.top_group_subsets), flat_m[order])
    np.testing.assert_array_equal(res.top_sizes, res.top_group_subsets.sum(axis=1))
    for m, cols in zip(flat_m[order], res.top_subsets):
        np.testing.assert_array_equal(cols, CG.columns_of(labels, int(m)))
    assert res.top_r_squared[0] == np.nanmax(res.r_squared)
    # rank 0 is the selection's winner on the same double
    sel = ls_spa_best_subsets_cv(X, y, reg, ids, groups=labels, _engine=CVGroupsTopOracleEngine())
    np.testing.assert_array_equal(res.r_squared[:, 0], sel.r_squared)
    np.testing.assert_array_equal(res.group_subsets[:, 0], sel.group_subsets)
    np.testing.assert_array_equal(res.subsets[:, 0], sel.subsets)
    np.testing.assert_array_equal(res.fold_r_squared[:, 0], sel.fold_r_squared)
    np.testing.assert_array_equal(res.theta[:, 0], sel.theta)
    assert res.best_size == sel.best_size and res.full_r_squared == sel.full_r_squared == u[-1]
    assert res.baseline_r_squared == sel.baseline_r_squared == res.r_squared[0, 0] == u[0]
    np.testing.assert_array_equal(res.best_group_subset, sel.best_group_subset)
    np.testing.assert_array_equal(res.best_subset, sel.best_subset)
    check_one_se(res)
    assert "cross-validation" in repr(res) and "one standard error" in repr(res) and "groups" in repr(res)
    # the column call is what it was: the column result class, the column engine calls
    from test_cv_top_host import CVTopOracleEngine
    col = CVTopOracleEngine()
    plain = ls_spa_top_subsets_cv(X[:, :7], y, reg, ids, T, _engine=col)
    assert type(plain) is TopSubsetsCVResults and col.calls == [("load", K, reg), ("top", 0, T), ("free",)]


def test_one_se_prefers_the_smaller_model():
    """tests/test_cv_top_host.py's constructed game with groups as players: g = 3 groups of two columns, K = 4.  All
    three groups win by 0.01 over {0}, but fold by fold the difference swings by +-0.03, so {0} is within one standard
    error and the one-standard-error model is group 0 alone: columns 0 and 3."""
    K = 4
    table = np.zeros((8, K))
    table[0b001] = [0.20, 0.20, 0.20, 0.20]
    table[0b010] = table[0b100] = [0.02, 0.01, 0.02, 0.01]
    table[0b011] = [0.13, 0.07, 0.14, 0.07]
    table[0b101] = [0.12, 0.06, 0.13, 0.06]
    table[0b110] = [0.03, 0.02, 0.03, 0.02]
    table[0b111] = [0.23, 0.17, 0.24, 0.17]
    X, y = R.data(6, 24, seed=1)
    labels = np.array([0, 1, 2, 0, 1, 2])
    res = ls_spa_top_group_subsets_cv(X, y, labels, folds=K, n_best=3, _engine=CVGroupsTopOracleEngine(table=table))
    assert res.best_size == 3 and res.one_se_size == 1 and res.one_se_group_subset.tolist() == [True, False, False]
    assert res.one_se_subset.tolist() == [True, False, False, True, False, False]
    d = table[0b111] - table[0b001]
    assert res.best_gap[1, 0] == res.r_squared[3, 0] - res.r_squared[1, 0] and abs(res.best_gap[1, 0] - 0.01) < 1e-15
    assert abs(res.best_gap_std_error[1, 0] - 2.0 * np.std(d, ddof=1)) < 1e-15
    assert res.within_one_se[1, 0] and not res.within_one_se[1, 1:].any()
    assert not res.within_one_se[0].any() and res.within_one_se[3, 0] and not res.within_one_se[2].any()
    assert res.baseline_r_squared == 0.0 and res.full_r_squared == res.r_squared[3, 0]
    check_one_se(res)


def test_warning_names_the_folds_and_a_dropped_size():
    K, T = 5, 3
    X, y, ids, labels, _, _ = CG.case("mixed", K)
    g = GT.n_groups(labels)
    with pytest.warns(RuntimeWarning, match=r"fold\(s\) 1, 3 "):
        res = ls_spa_top_group_subsets_cv(X, y, labels, folds=ids, n_best=T,
                                          _engine=CVGroupsTopOracleEngine(info=[0, 1, 0, 1, 0], drop=(2, g)))
    want = [0 if k in (2, g) else min(T, comb(g, k)) for k in range(g + 1)]
    assert res.n_models.tolist() == want
    assert np.isnan(res.r_squared[[2, g]]).all() and np.isnan(res.theta[[2, g]]).all()
    assert not res.subsets[[2, g]].any() and not res.group_subsets[[2, g]].any() and (res.n_columns[[2, g]] == 0).all()
    assert np.isnan(res.fold_r_squared[[2, g]]).all() and not res.within_one_se[[2, g]].any()
    assert res.best_size not in (2, g, -1)
    check_one_se(res)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ls_spa_top_group_subsets_cv(X, y, labels, folds=ids, n_best=T, _engine=CVGroupsTopOracleEngine())
        res = ls_spa_top_group_subsets_cv(X, y, labels, folds=ids, n_best=T,
                                          _engine=CVGroupsTopOracleEngine(drop=range(g + 1)))
    assert res.best_size == -1 and res.one_se_size == -1 and not res.best_subset.any() and not res.one_se_subset.any()
    assert not res.best_group_subset.any() and not res.one_se_group_subset.any() and np.isnan(res.baseline_r_squared)
    assert len(res.top_r_squared) == 0 and not res.within_one_se.any() and np.isnan(res.best_gap).all()


# ---- the margins of the GPU truth test's cases -------------------------------------------------------------------------
@pytest.mark.parametrize("K", GT.KS)
@pytest.mark.parametrize("name", GT.NAMES)
def test_truth_lists_have_a_clear_margin(name, K):
    """Inside every size's top-17 of the truth neighbours differ by more than MIN_GAP = 1e-9: the device's values are
    within 1e-11 of it, so its lists at every T <= 16 must hold the truth's masks in the truth's order."""
    _, _, _, labels, u, _ = GT.case(name, K)
    m = GT.margin(u, GT.n_groups(labels), GT.T_MAX)
    print(name, "K", K, "margin", m)
    assert m > GT.MIN_GAP
