"""The ridge path of the K-fold CV attribution (ls_spa_cv_path) -- CPU side: every refusal (raised without touching an
engine), the plan of the path's blocks and launches, and the driver through a NumPy double of the engine whose numbers
are the truth of tests/cv_ref.py / tests/cv_groups_ref.py: shapes, sums, the choice of the ridge value and the
one-standard-error fields."""
import warnings

import numpy as np
import pytest

import cv_groups_ref as GR
import cv_ref as R
from ls_spa import CVGroupPathResults, CVPathResults, SizeIncompatible, ls_spa_cv_path
from ls_spa._engine import debug_cv_path_groups_plan, debug_cv_path_plan, debug_subsets_top_plan

# the shapes of tests/test_gpu_cv_path.py's bitwise cases: (p, K) and (labels, K); their ridge values and blocks
GPU_COLUMN_CASES = [(p, K) for p in (5, 7, 13) for K in (2, 3, 5)]
GPU_REGS = [0.0, 1e-3, 0.1, 10.0, 0.1]
GPU_BLOCKS = [0, 1, 3, len(GPU_REGS)]


def gpu_group_labels(g, p, nb):
    """The labels of the GPU tests' grouped cases: nb baseline columns, the others dealt to g groups."""
    return np.concatenate([np.full(nb, -1), np.arange(p - nb) % g]).astype(np.int64)


GPU_GROUP_CASES = [(gpu_group_labels(3, 7, 2), 3), (gpu_group_labels(6, 40, 0), 2)]


# ---- refusals ----------------------------------------------------------------------------------------------------------
class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched ({name}) before the arguments were checked")


@pytest.mark.parametrize("groups", [None, np.array([-1, 0, 0, 1, 2])])
def test_regs_refusals_come_before_any_engine(groups):
    X, y = R.data(5, 30, seed=4)
    eng = Untouchable()
    with pytest.raises(ValueError, match="1 .. 256 ridge values"):
        ls_spa_cv_path(X, y, [], groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="one-dimensional"):
        ls_spa_cv_path(X, y, [[0.1, 0.2]], groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="one-dimensional"):
        ls_spa_cv_path(X, y, 0.1, groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="1 .. 256 ridge values"):
        ls_spa_cv_path(X, y, np.linspace(0, 1, 257), groups=groups, _engine=eng)
    with pytest.raises(ValueError, match=r"regs\[2\] = -0.5"):
        ls_spa_cv_path(X, y, [0.0, 1.0, -0.5, -1.0], groups=groups, _engine=eng)
    with pytest.raises(ValueError, match=r"regs\[1\] = nan"):
        ls_spa_cv_path(X, y, [0.0, np.nan], groups=groups, _engine=eng)
    with pytest.raises(ValueError, match=r"regs\[0\] = inf"):
        ls_spa_cv_path(X, y, [np.inf, 1.0], groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="numbers"):
        ls_spa_cv_path(X, y, ["a"], groups=groups, _engine=eng)


def test_data_refusals_come_before_any_engine():
    X, y = R.data(5, 30, seed=4)
    eng, regs = Untouchable(), [0.0, 0.1]
    with pytest.raises(SizeIncompatible):
        ls_spa_cv_path(X, y[:-1], regs, _engine=eng)
    with pytest.raises(ValueError, match="one-dimensional"):
        ls_spa_cv_path(X, y[:, None], regs, _engine=eng)
    with pytest.raises(ValueError, match="at most p = 32"):
        ls_spa_cv_path(np.ones((40, 33)), np.ones(40), regs, _engine=eng)
    for K in (1, 33, 0):
        with pytest.raises(ValueError, match="2 .. 32 folds"):
            ls_spa_cv_path(X, y, regs, folds=K, _engine=eng)
    with pytest.raises(ValueError, match="integer"):
        ls_spa_cv_path(X, y, regs, folds=2.5, _engine=eng)
    with pytest.raises(ValueError, match="empty"):
        ls_spa_cv_path(X[:3], y[:3], regs, folds=4, _engine=eng)
    labels = np.arange(30) % 3
    with pytest.raises(ValueError, match="0 .. K-1"):
        ls_spa_cv_path(X, y, regs, folds=np.where(labels == 0, -1, labels), _engine=eng)
    with pytest.raises(ValueError, match="fold 1 of 3 is empty"):
        ls_spa_cv_path(X, y, regs, folds=np.where(labels == 1, 0, labels), _engine=eng)
    with pytest.raises(ValueError, match="shape"):
        ls_spa_cv_path(X, y, regs, folds=labels[:-1], _engine=eng)
    with pytest.raises(ValueError, match="integers"):
        ls_spa_cv_path(X, y, regs, folds=labels + 0.5, _engine=eng)
    with pytest.raises(ValueError, match="identically zero"):
        ls_spa_cv_path(X, np.zeros(30), regs, _engine=eng)


def test_grouped_refusals_come_before_any_engine():
    X, y = R.data(6, 30, seed=4)
    eng, regs = Untouchable(), [0.0, 0.1]
    groups = np.array([-1, 0, 0, 1, 2, 2])
    with pytest.raises(SizeIncompatible):
        ls_spa_cv_path(X, y[:-1], regs, groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="one-dimensional"):
        ls_spa_cv_path(X, y[:, None], regs, groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="at most p = 64"):
        ls_spa_cv_path(np.ones((80, 65)), np.ones(80), regs, groups=np.arange(65) % 4, _engine=eng)
    for K in (1, 33, 0):
        with pytest.raises(ValueError, match="2 .. 32 folds"):
            ls_spa_cv_path(X, y, regs, folds=K, groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="empty"):
        ls_spa_cv_path(X[:3], y[:3], regs, folds=4, groups=groups, _engine=eng)
    ids = np.arange(30) % 3
    with pytest.raises(ValueError, match="0 .. K-1"):
        ls_spa_cv_path(X, y, regs, folds=np.where(ids == 0, -1, ids), groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="fold 1 of 3 is empty"):
        ls_spa_cv_path(X, y, regs, folds=np.where(ids == 1, 0, ids), groups=groups, _engine=eng)
    with pytest.raises(ValueError, match="identically zero"):
        ls_spa_cv_path(X, np.zeros(30), regs, groups=groups, _engine=eng)
    # the label errors of ls_spa_cv(groups=)
    with pytest.raises(ValueError, match="one label per column"):
        ls_spa_cv_path(X, y, regs, groups=groups[:-1], _engine=eng)
    with pytest.raises(ValueError, match="integer labels"):
        ls_spa_cv_path(X, y, regs, groups=groups + 0.5, _engine=eng)
    with pytest.raises(ValueError, match="below -1"):
        ls_spa_cv_path(X, y, regs, groups=np.array([-2, 0, 0, 1, 2, 2]), _engine=eng)
    with pytest.raises(ValueError, match="no group at all"):
        ls_spa_cv_path(X, y, regs, groups=np.full(6, -1), _engine=eng)
    with pytest.raises(ValueError, match="gap in its numbering"):
        ls_spa_cv_path(X, y, regs, groups=np.array([-1, 0, 0, 3, 2, 2]), _engine=eng)
    with pytest.raises(ValueError, match="at most g = 32"):
        ls_spa_cv_path(np.ones((80, 40)) + np.eye(80, 40), np.arange(80.0), regs, groups=np.arange(40), _engine=eng)


# ---- the plan ----------------------------------------------------------------------------------------------------------
def check_plan(plan, K, L, block):
    assert 1 <= plan["block"] <= L and (block == 0 or plan["block"] == min(block, L))
    assert plan["blocks"] == -(-L // plan["block"]) and plan["blocks"] * plan["block"] >= L
    assert 1 <= plan["steps"] <= plan["per"]
    assert 1 <= plan["reps"] <= plan["block"] * K
    # a launch stays within the library's bound on the subsets of a launch (one replicate always runs)
    assert plan["reps"] * plan["units"] * plan["steps"] <= plan["bound"] or plan["reps"] == 1
    # as many replicates as the bound leaves: one more would not fit, or the block has no more
    assert plan["reps"] == plan["block"] * K or (plan["reps"] + 1) * plan["units"] * plan["steps"] > plan["bound"]
    cuts = -(-plan["per"] // plan["steps"])
    want, left = 0, L
    while left > 0:
        n = min(plan["block"], left) * K
        want += -(-n // min(n, max(1, plan["bound"] // (plan["units"] * plan["steps"])))) * cuts
        left -= plan["block"]
    assert plan["launches"] == want


@pytest.mark.parametrize("L, block", [(1, 0), (4, 1), (5, 3), (32, 0), (256, 0), (256, 7)])
@pytest.mark.parametrize("K", [2, 5, 32])
@pytest.mark.parametrize("p", [1, 6, 7, 13, 19, 20, 24, 32])
def test_plan(p, K, L, block):
    plan = debug_cv_path_plan(p, K, L, block)
    one = debug_subsets_top_plan(p, 1)                       # the one-problem enumeration's cut: cv_shapley's of a fold
    assert plan["units"] == one["units"] == min(1 << max(p - 6, 0), 8192) and plan["per"] == one["per"]
    assert plan["steps"] == min(plan["per"], max(1, (1 << 20) // plan["units"])) and plan["bound"] == 1 << 20
    check_plan(plan, K, L, block)
    # the problems of a default block stay within 64 MiB
    if block == 0:
        assert plan["block"] * K * 8 * (2 * p * p + 2 * p + 1) <= 64 << 20 or plan["block"] == 1


@pytest.mark.parametrize("L, block", [(1, 0), (5, 3), (32, 0), (256, 0)])
@pytest.mark.parametrize("K", [2, 5, 32])
@pytest.mark.parametrize("labels", [gpu_group_labels(3, 7, 2), gpu_group_labels(6, 40, 0), gpu_group_labels(12, 64, 0),
                                    gpu_group_labels(16, 48, 0), GR.multi_labels()], ids=["3-7", "6-40", "12-64", "16-48",
                                                                                        "multi"])
def test_groups_plan(labels, K, L, block):
    from ls_spa._engine import debug_cv_groups_plan
    plan = debug_cv_path_groups_plan(labels, K, L, block)
    one = debug_cv_groups_plan(labels, 2)
    assert all(plan[k] == one[k] for k in ("gl", "gh", "ql", "nb", "units", "per"))
    assert plan["bound"] == min(1 << 20, one["launch_bound"])
    assert plan["steps"] == min(plan["per"], max(1, one["launch_bound"] // plan["units"]))
    check_plan(plan, K, L, block)


def test_plan_refusals():
    for p, K, L, block in [(0, 5, 4, 0), (33, 5, 4, 0), (8, 1, 4, 0), (8, 33, 4, 0), (8, 5, 0, 0), (8, 5, 257, 0),
                           (8, 5, 4, -1)]:
        with pytest.raises(ValueError):
            debug_cv_path_plan(p, K, L, block)
    ok = np.array([-1, 0, 0, 1, 2, 2])
    for K, L, block in [(1, 4, 0), (33, 4, 0), (5, 0, 0), (5, 257, 0), (5, 4, -1)]:
        with pytest.raises(ValueError):
            debug_cv_path_groups_plan(ok, K, L, block)
    for bad in (np.array([0, 2, 2]), np.array([-1, -1]), np.arange(33), np.zeros(65, dtype=int), np.array([-2, 0])):
        with pytest.raises(ValueError):
            debug_cv_path_groups_plan(bad, 5, 4, 0)


def test_gpu_cases_are_cut_into_several_blocks_and_launches():
    """What tests/test_gpu_cv_path.py relies on: its forced blocks of 1 and 3 ridge values cut the path of
    len(GPU_REGS) values into several blocks, and so into several launches."""
    L = len(GPU_REGS)
    for block in (1, 3):
        for p, K in GPU_COLUMN_CASES:
            plan = debug_cv_path_plan(p, K, L, block)
            assert plan["blocks"] == -(-L // block) > 1 and plan["launches"] >= plan["blocks"] > 1
        for labels, K in GPU_GROUP_CASES:
            plan = debug_cv_path_groups_plan(labels, K, L, block)
            assert plan["blocks"] == -(-L // block) > 1 and plan["launches"] >= plan["blocks"] > 1
    for p, K in GPU_COLUMN_CASES:
        assert debug_cv_path_plan(p, K, L, 0)["blocks"] == 1 == debug_cv_path_plan(p, K, L, L)["blocks"]


# ---- the driver on a test double ---------------------------------------------------------------------------------------
class PathOracleEngine:
    """What ls_spa_cv_path asks of an engine, computed ridge value by ridge value by tests/cv_ref.py and
    tests/cv_groups_ref.py (rounded to fp64).  info [L][K]: the info words it reports."""

    def __init__(self, info=None):
        self.calls, self._info = [], info

    def cv_load(self, X, y, fold_ids, K, reg):
        self.calls.append(("load", K, reg))
        self._data = X, y, np.asarray(fold_ids), K

    def cv_groups_load(self, X, y, fold_ids, K, reg):
        self.calls.append(("groups_load", K, reg))
        self._data = X, y, np.asarray(fold_ids), K

    def cv_free(self):
        self.calls.append(("free",))

    def _bits(self, L, K):
        return np.zeros((L, K), dtype=np.int32) if self._info is None else np.asarray(self._info, dtype=np.int32)

    @staticmethod
    def _sum(fold):
        total = fold[0].copy()
        for f in range(1, len(fold)):
            total = total + fold[f]
        return total

    def cv_path_shapley(self, regs, block=0):
        X, y, ids, K = self._data
        p = X.shape[1]
        self.calls.append(("path", tuple(regs)))
        phi, fold, r2 = [], [], []
        for reg in regs:
            _, vf = R.cv_values(X, y, ids, K, float(reg))
            fold.append(np.array([R.shapley(vf[:, f], p).astype(np.float64) for f in range(K)]))
            phi.append(self._sum(fold[-1]))
            r2.append(vf[-1].astype(np.float64))
        return np.array(phi), np.array(fold), np.array(r2), self._bits(len(regs), K)

    def cv_path_groups_shapley(self, labels, regs, block=0):
        X, y, ids, K = self._data
        g = int(np.max(labels)) + 1
        self.calls.append(("groups_path", tuple(regs)))
        phi, fold, r2, base = [], [], [], []
        for reg in regs:
            _, uf = GR.cv_values(X, y, ids, K, labels, float(reg))
            fold.append(np.array([GR.shapley(uf[:, f], g) for f in range(K)]))
            phi.append(self._sum(fold[-1]))
            r2.append(uf[-1].copy())
            base.append(uf[0].copy())
        return np.array(phi), np.array(fold), np.array(r2), np.array(base), self._bits(len(regs), K)


def check_choice(res):
    """best_index and the one-standard-error fields from the result's own per-fold values, restated."""
    r2, fold, regs = res.r_squared, res.fold_r_squared, res.regs
    K = fold.shape[1]
    b = res.best_index
    assert r2[b] == np.nanmax(r2) and regs[b] == max(regs[r2 == r2[b]]) and res.best_reg == regs[b]
    d = fold[b][None, :] - fold
    np.testing.assert_allclose(res.best_gap, d.sum(axis=1), rtol=0, atol=1e-15)
    np.testing.assert_allclose(res.best_gap_std_error, np.sqrt(K) * d.std(axis=1, ddof=1), rtol=1e-12, atol=0)
    np.testing.assert_array_equal(res.within_one_se, res.best_gap <= res.best_gap_std_error)
    assert res.within_one_se[b] and res.best_gap[b] == 0.0 and res.best_gap_std_error[b] == 0.0
    assert res.within_one_se[res.one_se_index] and res.one_se_reg == regs[res.one_se_index] == max(regs[res.within_one_se])
    assert res.one_se_reg >= res.best_reg


def test_ls_spa_cv_path_on_the_double():
    p, K, n = 6, 4, 50
    X, y = R.data(p, n, seed=6)
    regs = [0.3, 0.0, 1e-2, 5.0, 0.3]
    eng = PathOracleEngine()
    res = ls_spa_cv_path(X, y, regs, K, seed=3, _engine=eng)
    L = len(regs)
    assert isinstance(res, CVPathResults) and eng.calls == [("load", K, 0.3), ("path", tuple(regs)), ("free",)]
    ids = R.fold_ids(n, K, seed=3)
    np.testing.assert_array_equal(res.fold_ids, ids)
    np.testing.assert_array_equal(res.regs, regs)
    assert res.attribution.shape == (L, p) and res.fold_attribution.shape == (L, K, p)
    assert res.r_squared.shape == (L,) and res.fold_r_squared.shape == (L, K) and res.theta.shape == (L, p)
    assert res.best_gap.shape == res.best_gap_std_error.shape == res.within_one_se.shape == (L,)
    for l, reg in enumerate(regs):
        v, _ = R.cv_values(X, y, ids, K, reg)
        np.testing.assert_allclose(res.attribution[l], R.shapley(v, p).astype(np.float64), rtol=0, atol=1e-14)
        assert abs(res.r_squared[l] - float(v[-1])) < 1e-14
        G = X.T @ X / n + reg * np.eye(p)
        np.testing.assert_allclose(res.theta[l], np.linalg.solve(G, X.T @ y / n), rtol=1e-12)
    np.testing.assert_allclose(res.attribution.sum(axis=1), res.r_squared, rtol=0, atol=1e-13)
    np.testing.assert_allclose(res.fold_r_squared.sum(axis=1), res.r_squared, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(res.attribution[0], res.attribution[4])             # the repeated value
    check_choice(res)
    assert "ridge values" in repr(res) and "one standard error" in repr(res)
    one = ls_spa_cv_path(X, y, [0.3], K, seed=3, _engine=PathOracleEngine())         # L = 1
    np.testing.assert_array_equal(one.attribution[0], res.attribution[0])
    assert one.best_index == one.one_se_index == 0 and one.within_one_se.tolist() == [True]
    same = ls_spa_cv_path(X, y, np.array(regs, dtype=np.float32).astype(np.float64), ids, _engine=PathOracleEngine())
    np.testing.assert_array_equal(same.fold_ids, ids)                                  # the labels taken as given


def test_ls_spa_cv_path_groups_on_the_double():
    labels = gpu_group_labels(3, 7, 2)
    p, g, K, n = 7, 3, 3, 60
    X, y = R.data(p, n, seed=8)
    regs = [0.0, 0.5, 1e-3]
    eng = PathOracleEngine()
    res = ls_spa_cv_path(X, y, regs, K, groups=labels, _engine=eng)
    L = len(regs)
    assert isinstance(res, CVGroupPathResults)
    assert eng.calls == [("groups_load", K, 0.0), ("groups_path", tuple(regs)), ("free",)]
    assert res.attribution.shape == (L, g) and res.fold_attribution.shape == (L, K, g) and res.theta.shape == (L, p)
    assert res.baseline_r_squared.shape == (L,) and res.fold_baseline_r_squared.shape == (L, K)
    assert res.r_squared.shape == (L,) and res.fold_r_squared.shape == (L, K)
    for l, reg in enumerate(regs):
        u, _ = GR.cv_values(X, y, res.fold_ids, K, labels, reg)
        np.testing.assert_allclose(res.attribution[l], GR.shapley(u, g), rtol=0, atol=1e-13)
        assert abs(res.r_squared[l] - u[-1]) < 1e-14 and abs(res.baseline_r_squared[l] - u[0]) < 1e-14
    np.testing.assert_allclose(res.attribution.sum(axis=1), res.r_squared - res.baseline_r_squared, rtol=0, atol=1e-13)
    np.testing.assert_allclose(res.fold_baseline_r_squared.sum(axis=1), res.baseline_r_squared, rtol=0, atol=1e-15)
    assert (res.baseline_r_squared > 0).all()
    check_choice(res)
    assert "groups" in repr(res)


class HandMadeEngine(PathOracleEngine):
    """The double with per-fold R^2 values given by hand (the attributions are of no interest here)."""

    def __init__(self, r2_fold, info=None):
        super().__init__(info)
        self._r2 = np.asarray(r2_fold, dtype=np.float64)

    def cv_path_shapley(self, regs, block=0):
        L, K = self._r2.shape
        p = self._data[0].shape[1]
        return np.zeros((L, p)), np.zeros((L, K, p)), self._r2.copy(), self._bits(L, K)


def hand_made(regs, r2_fold, info=None):
    X, y = R.data(3, 12, seed=1)
    K = np.shape(r2_fold)[1]
    return ls_spa_cv_path(X, y, regs, K, _engine=HandMadeEngine(r2_fold, info))


def test_best_index_tie_rule():
    # rows 1 and 3 tie exactly for the best sum: the larger ridge value wins, wherever it stands
    fold = [[0.1, 0.2], [0.25, 0.25], [0.2, 0.1], [0.25, 0.25]]
    res = hand_made([0.0, 0.5, 1.0, 2.0], fold)
    assert res.best_index == 3 and res.best_reg == 2.0
    res = hand_made([0.0, 2.0, 1.0, 0.5], fold)
    assert res.best_index == 1 and res.best_reg == 2.0
    res = hand_made([0.0, 0.5, 1.0, 0.5], fold)                 # the same ridge value twice: the earlier row
    assert res.best_index == 1 and res.one_se_index == 1
    # NaN rows are skipped, in the choice and in the one-standard-error fields
    nan = [[np.nan, 0.9], [0.25, 0.25], [np.nan, np.nan], [0.2, 0.2]]
    res = hand_made([0.0, 0.5, 9.0, 2.0], nan)
    assert res.best_index == 1 and np.isnan(res.best_gap[[0, 2]]).all() and not res.within_one_se[[0, 2]].any()
    assert res.one_se_index in (1, 3)
    res = hand_made([0.0, 1.0], [[np.nan, 0.1], [0.2, np.nan]])
    assert res.best_index == -1 and res.one_se_index == -1 and np.isnan(res.best_reg) and np.isnan(res.one_se_reg)
    assert np.isnan(res.best_gap).all() and not res.within_one_se.any()


def test_one_standard_error_fields():
    regs = [0.0, 0.1, 1.0, 10.0]
    fold = np.array([[0.20, 0.22, 0.18],        # b - this: d = (0.02, 0.02, 0.02): gap 0.06, std 0: outside
                     [0.22, 0.24, 0.20],        # the best
                     [0.24, 0.18, 0.22],        # d = (-0.02, 0.06, -0.02): gap 0.02, se sqrt(3) std(d) = 0.08: within
                     [0.10, 0.30, 0.05]])       # d = (0.12, -0.06, 0.15): gap 0.21, se 0.197: outside
    res = hand_made(regs, fold)
    assert res.best_index == 1 and res.best_reg == 0.1
    np.testing.assert_allclose(res.best_gap, [0.06, 0.0, 0.02, 0.21], rtol=0, atol=1e-15)
    d = fold[1][None, :] - fold
    np.testing.assert_allclose(res.best_gap_std_error, np.sqrt(3) * d.std(axis=1, ddof=1), rtol=1e-13, atol=0)
    assert abs(res.best_gap_std_error[2] - 0.08) < 1e-15 and res.best_gap_std_error[1] == 0.0
    assert res.within_one_se.tolist() == [False, True, True, False]
    assert res.one_se_index == 2 and res.one_se_reg == 1.0
    # the best model is itself the largest ridge value: it is its own one-standard-error choice
    res = hand_made(regs, fold[[0, 2, 3, 1]])
    assert res.best_index == 3 and res.one_se_index == 3 and res.one_se_reg == 10.0 == res.best_reg
    assert res.within_one_se.tolist() == [False, True, False, True]
    # ... and in the caller's order, whatever it is: the largest qualifying VALUE, not the last row
    res = hand_made([1.0, 0.1, 10.0, 0.0], fold[[2, 1, 3, 0]])
    assert res.best_index == 1 and res.one_se_index == 0 and res.one_se_reg == 1.0


def test_warning_names_the_ridge_values_and_their_folds():
    fold = np.full((3, 4), 0.2)
    info = [[0, 1, 0, 1], [0, 0, 0, 0], [1, 0, 0, 0]]
    with pytest.warns(RuntimeWarning, match=r"ridge value 0 \(regs\[0\]\): fold\(s\) 1, 3; ridge value 0.5 "
                                            r"\(regs\[2\]\): fold\(s\) 0;"):
        hand_made([0.0, 0.1, 0.5], fold, info)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        hand_made([0.0, 0.1, 0.5], fold)
