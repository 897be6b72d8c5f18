"""K-fold cross-validation over groups of columns -- CPU side: the cases of tests/cv_groups_ref.py vetted (the gap
between winner and runner-up, the truth against a restatement on explicit rows), the plan of the selection kernel against
the one-problem plan, every refusal (raised without touching an engine), and the drivers through a NumPy double of the
engine whose numbers are that truth."""
import warnings

import numpy as np
import pytest

import cv_groups_ref as CG
import cv_ref as R
import group_best_ref as GB
from ls_spa import (CVBestGroupSubsetsResults, CVGroupResults, SizeIncompatible, ls_spa_best_subsets_cv, ls_spa_cv)
from ls_spa._engine import debug_cv_groups_plan, debug_groups_best_plan

GPU_RUNS = [(name, K, CG.N_ROWS) for name in CG.NAMES for K in CG.KS] + [CG.WIDE]


# ---- the cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, K, n", GPU_RUNS)
def test_cases_have_a_clear_winner_of_every_size(name, K, n):
    X, y, ids, labels, u, uf = CG.case(name, K, n)
    g = int(labels.max()) + 1
    assert X.shape[1] == len(labels) and min(np.bincount(ids)) >= 1
    assert n - max(np.bincount(ids)) > X.shape[1]              # every training fold has more rows than columns
    best, masks, found, runner = CG.best(u, g)
    gap = (best - runner)[np.isfinite(runner)]
    print(name, K, "smallest gap", gap.min() if len(gap) else None)
    assert found.all() and (gap > CG.MIN_GAP).all()
    np.testing.assert_array_equal(u, CG.seq_sum(uf))


@pytest.mark.parametrize("name", CG.NAMES)
def test_truth_against_lstsq_on_explicit_rows(name):
    K = 5
    X, y, ids, labels, u, uf = CG.case(name, K)
    g = int(labels.max()) + 1
    rng = np.random.default_rng(3)
    picks = np.unique(np.concatenate([[0, (1 << g) - 1], rng.integers(0, 1 << g, size=12)]))
    for m in picks:
        want, folds = CG.lstsq_value(X, y, ids, K, labels, int(m))
        assert abs(u[m] - want) < 1e-11 and np.abs(uf[m] - np.array(folds)).max() < 1e-11, (name, m)
    phi = CG.shapley(u, g)
    assert abs(phi.sum() - (u[-1] - u[0])) < 1e-12             # efficiency: what the groups add to the baseline
    per_fold = sum(CG.shapley(uf[:, f], g) for f in range(K))
    assert np.abs(phi - per_fold).max() < 1e-13                # linearity in the game


def test_tie_cases_tie_exactly():
    for run in CG.TIE_RUNS:
        X, y, ids, labels, u = CG.tie_case(run)
        lab = CG.TIE_RUNS[run]
        inside = [m for m in range(32) if not m & ((1 << lab["d"]) | (1 << lab["e"]))]
        assert (u[inside] == 0.0).all()                        # exactly: g is 0 on the columns of a, b, c
        others = [m for m in range(32) if m not in inside]
        assert (u[others] < -0.05).all()                       # far below the tie
        _, masks, found, _ = CG.best(u, 5)
        assert found.all() and list(masks[1:4]) == CG.tie_winners(run)


# ---- the plan ----------------------------------------------------------------------------------------------------------
LAYOUTS = {name: GB.case_labels(name) for name in GB.CASES}
LAYOUTS.update({name: lab for name, (lab, _) in GB.PLANTED.items()})
LAYOUTS["multi"] = CG.multi_labels()
LAYOUTS["p64"] = np.arange(64) % 32


@pytest.mark.parametrize("K", [2, 5, 32])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_plan(name, K):
    labels = LAYOUTS[name]
    plan, one = debug_cv_groups_plan(labels, K), debug_groups_best_plan(labels)
    for key in ("gl", "gh", "ql", "nb", "units", "per"):
        assert plan[key] == one[key], key
    p = len(labels)
    rows = (plan["nb"] + plan["ql"] + 1) + (p - plan["nb"] - plan["ql"] + 1) // 2
    bound = max(1, (1 << 26) // (rows * rows))                 # the one-problem launch's high subsets (lsspa_api.hip)
    assert plan["launch_bound"] == bound
    assert one["launches"] == -(-one["per"] // min(one["per"], max(1, bound // one["units"])))
    assert plan["steps"] == min(plan["per"], max(1, bound // (plan["units"] * K)))
    assert plan["launches"] == -(-plan["per"] // plan["steps"])
    assert plan["workgroup"] == 256
    assert plan["lds_bytes"] == plan["lds_bytes_one_problem"] and 40000 < plan["lds_bytes"] <= 80 * 1024


def test_plan_of_the_multi_launch_case():
    plan = debug_cv_groups_plan(CG.multi_labels(), CG.MULTI_K)
    print(plan)
    assert plan["gl"] == 3 and plan["ql"] == 5 and plan["gh"] == 15 and plan["nb"] == CG.MULTI_NB
    assert plan["units"] == 8192 and plan["per"] == 4 and plan["steps"] == 2 and plan["launches"] == 2


def test_plan_refusals():
    ok = np.arange(6) % 3
    for K in (1, 33, 0):
        with pytest.raises(ValueError):
            debug_cv_groups_plan(ok, K)
    for bad in (np.array([0, 2, 2]), np.array([-1, -1]), np.arange(33), np.zeros(65, dtype=int), np.array([-2, 0])):
        with pytest.raises(ValueError):
            debug_cv_groups_plan(bad, 5)


# ---- refusals ----------------------------------------------------------------------------------------------------------
class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched ({name}) before the arguments were checked")


@pytest.mark.parametrize("call", [ls_spa_cv, ls_spa_best_subsets_cv])
def test_refusals_come_before_any_engine(call):
    X, y = R.data(6, 30, seed=4)
    eng = Untouchable()
    groups = np.array([-1, 0, 0, 1, 2, 2])
    with pytest.raises(SizeIncompatible):
        call(X, y[:-1], groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="one-dimensional"):
        call(X, y[:, None], groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="at most p = 64"):
        call(np.ones((80, 65)), np.ones(80), groups=np.arange(65) % 4, _engine=eng)
    with pytest.raises(ValueError, match="at most p = 32"):          # without groups the column limit stays
        call(np.ones((40, 33)), np.ones(40), _engine=eng)
    for K in (1, 33, 0):
        with pytest.raises(ValueError, match="2 .. 32 folds"):
            call(X, y, folds=K, groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="empty"):
        call(X[:3], y[:3], folds=4, groups=groups, _engine=eng)
    ids = np.arange(30) % 3
    with pytest.raises(ValueError, match="0 .. K-1"):
        call(X, y, folds=np.where(ids == 0, -1, ids), groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="fold 1 of 3 is empty"):
        call(X, y, folds=np.where(ids == 1, 0, ids), groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="identically zero"):
        call(X, np.zeros(30), groups=groups, _engine=eng)
    # the label errors of ls_spa(groups=)
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
    with pytest.raises(ValueError, match="at most g = 32"):
        call(np.ones((80, 40)) + np.eye(80, 40), np.arange(80.0), groups=np.arange(40), _engine=eng)


def test_include_with_groups_is_refused():
    X, y = R.data(6, 30, seed=4)
    with pytest.raises(ValueError, match="include= cannot be combined with groups="):
        ls_spa_best_subsets_cv(X, y, include=[0], groups=np.array([-1, 0, 0, 1, 2, 2]), _engine=Untouchable())


# ---- the drivers on a test double --------------------------------------------------------------------------------------
class CVGroupsOracleEngine:
    """What the grouped cross-validation drivers ask of an engine, computed by tests/cv_groups_ref.py.  info: the folds'
    info words it reports; drop: sizes it reports as not found."""
    precision = "float64"
    p = 0

    def __init__(self, info=None, drop=()):
        self.calls, self._info, self._drop = [], info, tuple(drop)

    def cv_groups_load(self, X, y, fold_ids, K, reg):
        self.calls.append(("load", K, reg))
        self._data, self._K = (np.asarray(X), np.asarray(y), np.asarray(fold_ids), K, reg), K

    def cv_free(self):
        self.calls.append(("free",))

    def _bits(self):
        return np.zeros(self._K, dtype=np.int32) if self._info is None else np.asarray(self._info, dtype=np.int32)

    def _table(self, labels):
        X, y, ids, K, reg = self._data
        labels = np.asarray(labels)
        assert labels.dtype == np.int32 and len(labels) == X.shape[1]
        return CG.cv_values(X, y, ids, K, labels, reg) + (int(labels.max()) + 1,)

    def cv_groups_shapley(self, labels):
        self.calls.append(("shapley",))
        u, uf, g = self._table(labels)
        fold = np.array([CG.shapley(uf[:, f], g) for f in range(self._K)])
        return CG.seq_sum(fold.T), fold, uf[-1].copy(), uf[0].copy(), self._bits()

    def cv_groups_best(self, labels, steps=0):
        self.calls.append(("best",))
        u, uf, g = self._table(labels)
        best, masks, found, _ = CG.best(u, g)
        for k in self._drop:
            best[k], masks[k], found[k] = np.nan, 0, False
        u_fold = np.full((g + 1, self._K), np.nan)
        u_fold[found] = uf[masks[found].astype(np.int64)]
        return best, masks, found, u_fold, self._bits()

    def debug_cv_group_values(self, labels, masks, folds=True):
        u, uf, _ = self._table(labels)
        m = np.asarray(masks).astype(np.int64)
        return u[m], (uf[m] if folds else None)

    def set_flags(self, flags):
        pass


def test_ls_spa_cv_groups_on_the_double():
    K = 5
    X, y, ids, labels, u, uf = CG.case("mixed", K)
    g, n, p = int(labels.max()) + 1, len(y), len(labels)
    eng = CVGroupsOracleEngine()
    res = ls_spa_cv(X, y, 0.0, ids, groups=labels, _engine=eng)
    assert isinstance(res, CVGroupResults) and eng.calls == [("load", K, 0.0), ("shapley",), ("free",)]
    np.testing.assert_array_equal(res.fold_ids, ids)
    np.testing.assert_allclose(res.attribution, CG.shapley(u, g), rtol=0, atol=1e-14)
    assert res.attribution.shape == (g,) and res.fold_attribution.shape == (K, g)
    assert res.fold_r_squared.shape == (K,) and res.fold_baseline_r_squared.shape == (K,)
    assert abs(res.r_squared - u[-1]) < 1e-14 and abs(res.baseline_r_squared - u[0]) < 1e-14
    assert abs(res.attribution.sum() - (res.r_squared - res.baseline_r_squared)) < 1e-13
    np.testing.assert_allclose(res.theta, np.linalg.solve(X.T @ X / n, X.T @ y / n), rtol=1e-11)
    assert res.theta.shape == (p,) and "groups" in repr(res)
    by_count = ls_spa_cv(X, y, folds=K, seed=CG.FOLD_SEED, groups=list(labels), _engine=CVGroupsOracleEngine())
    np.testing.assert_array_equal(by_count.attribution, res.attribution)


def test_ls_spa_best_subsets_cv_groups_on_the_double():
    K = 2
    X, y, ids, labels, u, uf = CG.case("nine", K)
    g, n, p = int(labels.max()) + 1, len(y), len(labels)
    eng = CVGroupsOracleEngine()
    res = ls_spa_best_subsets_cv(X, y, 0.0, ids, groups=labels, _engine=eng)
    assert isinstance(res, CVBestGroupSubsetsResults) and eng.calls[1] == ("best",) and eng.calls[-1] == ("free",)
    assert res.sizes.tolist() == list(range(g + 1)) and res.group_subsets.shape == (g + 1, g)
    assert res.subsets.shape == res.theta.shape == (g + 1, p) and res.fold_r_squared.shape == (g + 1, K)
    best, masks, found, _ = CG.best(u, g)
    np.testing.assert_allclose(res.r_squared, best, rtol=0, atol=1e-14)
    np.testing.assert_array_equal(res.r_squared, CG.seq_sum(res.fold_r_squared))
    G, gv = X.T @ X / n, X.T @ y / n
    for k in range(g + 1):
        assert sum(1 << int(j) for j in np.nonzero(res.group_subsets[k])[0]) == masks[k]
        np.testing.assert_array_equal(res.subsets[k], CG.columns_of(labels, masks[k]))
        cols = np.nonzero(res.subsets[k])[0]
        np.testing.assert_allclose(res.theta[k, cols], np.linalg.solve(G[np.ix_(cols, cols)], gv[cols]), rtol=1e-11)
        assert (res.theta[k, ~res.subsets[k]] == 0.0).all()
    np.testing.assert_array_equal(res.n_columns, res.subsets.sum(axis=1))
    assert res.group_subsets.sum(axis=1).tolist() == res.sizes.tolist()
    assert res.best_size == int(np.argmax(res.r_squared)) and "Best model" in repr(res)
    np.testing.assert_array_equal(res.best_group_subset, res.group_subsets[res.best_size])
    np.testing.assert_array_equal(res.best_subset, res.subsets[res.best_size])
    assert abs(res.full_r_squared - u[-1]) < 1e-14 and res.baseline_r_squared == res.r_squared[0]
    assert abs(res.baseline_r_squared - u[0]) < 1e-14


def test_warning_names_the_folds_and_nan_rows():
    K = 5
    X, y, ids, labels, u, uf = CG.case("mixed", K)
    g = int(labels.max()) + 1
    with pytest.warns(RuntimeWarning, match=r"fold\(s\) 1, 3 "):
        res = ls_spa_best_subsets_cv(X, y, folds=ids, groups=labels,
                                     _engine=CVGroupsOracleEngine(info=[0, 1, 0, 1, 0], drop=(2, g)))
    assert np.isnan(res.r_squared[[2, g]]).all() and np.isnan(res.theta[[2, g]]).all()
    assert not res.subsets[[2, g]].any() and not res.group_subsets[[2, g]].any()
    assert np.isnan(res.fold_r_squared[[2, g]]).all()
    keep = [k for k in range(g + 1) if k not in (2, g)]
    assert res.best_size in keep and not np.isnan(res.r_squared[keep]).any()
    with pytest.warns(RuntimeWarning, match=r"fold\(s\) 0 "):
        ls_spa_cv(X, y, folds=ids, groups=labels, _engine=CVGroupsOracleEngine(info=[1, 0, 0, 0, 0]))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ls_spa_cv(X, y, folds=ids, groups=labels, _engine=CVGroupsOracleEngine())
    res = ls_spa_best_subsets_cv(X, y, folds=ids, groups=labels, _engine=CVGroupsOracleEngine(drop=range(g + 1)))
    assert res.best_size == -1 and not res.best_subset.any() and not res.best_group_subset.any()
    assert np.isnan(res.baseline_r_squared)
