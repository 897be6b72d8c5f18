"""ls_spa_owen: exact Owen values, the attribution of every column with the groups as coalition structure -- CPU side.

The truth of tests/owen_ref.py pinned by what does not involve the GPU: the two-level formula against the mean over all
group-contiguous orderings, all-singleton groups and a single group against the ungrouped Shapley value, the groups'
sums against the group game.  Then the reach of the GPU cases through the library's host-only planner, and the driver's
plumbing through a test double of the engine whose Owen values are that truth."""
import numpy as np
import pytest

from ls_spa import OwenResults, _driver, ls_spa, ls_spa_owen
from ls_spa._engine import debug_owen_plan
from owen_ref import (BIG_CASE, BIG_PLAN, GPU_CASES, owen_by_orderings, owen_values, owen_values_fast)
from test_groups_host import GroupsOracleEngine, group_shapley, labels_of, schur_problem, value
from test_subsets_host import data, exact_shapley, gram_problem


# ---- the truth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes, nb", [([2, 1, 3], 0), ([3, 3], 2), ([1, 1, 4], 3)])
def test_the_two_truths_agree(sizes, nb):
    labels = labels_of(sizes, nb, seed=len(sizes))
    prob = gram_problem(*data(len(labels), seed=80 + len(labels)), reg=0.05)
    np.testing.assert_allclose(owen_values(*prob, labels), owen_by_orderings(*prob, labels), rtol=0, atol=1e-13)


@pytest.mark.parametrize("p", [1, 4, 7])
def test_singletons_give_the_ungrouped_shapley_value(p):
    prob = gram_problem(*data(p, seed=p), reg=0.05)
    np.testing.assert_allclose(owen_values(*prob, np.arange(p)), exact_shapley(*prob), rtol=0, atol=1e-13)


@pytest.mark.parametrize("nb", [0, 2])
def test_one_group_gives_the_shapley_value_of_its_columns_with_the_baseline_eliminated(nb):
    labels = labels_of([6], nb, seed=3)
    prob = gram_problem(*data(len(labels), seed=90 + nb), reg=0.02)
    red = schur_problem(*prob, labels) if nb else prob + (labels,)
    got = owen_values(*prob, labels)
    np.testing.assert_allclose(got[labels == 0], exact_shapley(*red[:5]), rtol=0, atol=1e-13)
    assert (got[labels == -1] == 0.0).all()


@pytest.mark.parametrize("sizes, nb", [([2, 1, 3], 0), ([3, 3], 2), ([1, 1, 4], 3), ([2, 4, 1, 3], 1)])
def test_group_sums_and_efficiency(sizes, nb):
    labels = labels_of(sizes, nb, seed=5)
    prob = gram_problem(*data(len(labels), seed=100 + len(labels)))
    ow = owen_values(*prob, labels)
    phi = group_shapley(*prob, labels)
    np.testing.assert_allclose([ow[labels == k].sum() for k in range(len(sizes))], phi, rtol=0, atol=1e-13)
    total = value(*prob, np.arange(len(labels))) - value(*prob, np.nonzero(labels == -1)[0])
    assert abs(ow.sum() - total) < 1e-13


def test_the_owen_value_is_neither_the_ungrouped_value_nor_an_even_split():
    labels = labels_of([3, 2, 1])
    prob = gram_problem(*data(6, seed=60))
    ow = owen_values(*prob, labels)
    assert np.abs(ow - exact_shapley(*prob)).max() > 1e-4
    assert np.abs(ow[:3] - group_shapley(*prob, labels)[0] / 3).max() > 1e-4


@pytest.mark.parametrize("sizes, nb", [([2, 1, 3], 0), ([3, 2, 4], 2), ([4, 1, 1, 5], 3), ([5, 5, 5, 5], 4)])
def test_the_fast_truth_is_the_truth(sizes, nb):
    labels = labels_of(sizes, nb, seed=7)
    p = len(labels)
    for reg in (0.0, 0.1):
        prob = gram_problem(*data(p, n=4 * p + 8, m=3 * p + 5, seed=110 + p), reg=reg)
        np.testing.assert_allclose(owen_values_fast(*prob, labels), owen_values(*prob, labels), rtol=0, atol=1e-13)


# ---- the reach of the GPU cases (host-only planner of the library) ------------------------------------------------------
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_gpu_cases_reach_what_they_claim(name):
    labels, claims = GPU_CASES[name]
    plan = debug_owen_plan(labels)
    g = int(labels.max()) + 1
    size = np.bincount(labels[labels >= 0])
    assert len(plan) == g
    for k, row in enumerate(plan):
        assert row["players"] == g - 1 + size[k] and row["gl"] + row["gh"] == row["players"]
        assert row["inner_low"] + row["inner_high"] == size[k] and row["high_subsets"] == 1 << row["gh"]
        assert (row["launches"] == 0) == (size[k] == 1)
    for k, want in claims.items():
        assert {f: plan[k][f] for f in want} == want, (k, plan[k])


def test_the_big_case_has_two_launches_for_the_target_of_8():
    plan = debug_owen_plan(BIG_CASE)
    for k, want in BIG_PLAN.items():
        assert {f: plan[k][f] for f in want} == want, (k, plan[k])
    assert plan[14]["launches"] >= 2


@pytest.mark.parametrize("labels", [
    [0, 0, 2, 2, -1, -1],                          # an empty group
    [0, 0, 1, 1, -2, -1],                          # a label below -1
    [-1] * 6,                                      # no group
    np.minimum(np.arange(40), 32),                 # 33 groups
    np.arange(65) % 8,                             # 65 columns
    np.minimum(np.arange(60), 30),                 # 31 groups, the last of 30 columns: 60 players
])
def test_planner_refuses_what_the_call_refuses(labels):
    with pytest.raises(ValueError, match="lsspa_debug_owen_plan"):
        debug_owen_plan(labels)


# ---- driver plumbing on a test double ----------------------------------------------------------------------------------
class OwenOracleEngine(GroupsOracleEngine):
    """GroupsOracleEngine with the Owen call, computed by the truth."""

    def __init__(self, info=0):
        super().__init__(info)
        self.owen_calls = []

    def groups_owen(self, labels):
        assert isinstance(labels, np.ndarray) and labels.dtype == np.int32 and labels.shape == (self.p,)
        self.owen_calls.append(labels.copy())
        G, g, H, h = self.gram()
        return (owen_values(G, g, H, h, self.y_norm_sq, labels), group_shapley(G, g, H, h, self.y_norm_sq, labels),
                self._info)


@pytest.mark.parametrize("kind", ["int64", "int8", "list"])
@pytest.mark.parametrize("m", [40, 5])             # 5 test rows for 9 columns: the test factor is kept (rect mode)
def test_result_fields(kind, m):
    labels = labels_of([2, 3, 1], 3, seed=7)
    p = len(labels)
    d = data(p, m=m, seed=70)
    eng = OwenOracleEngine()
    res = ls_spa_owen(*d, labels.tolist() if kind == "list" else labels.astype(kind), reg=0.1, _engine=eng)
    ref = ls_spa(*d, reg=0.1, method="subsets", groups=labels, _engine=GroupsOracleEngine())
    assert isinstance(res, OwenResults) and "Owen" in repr(res)
    assert len(eng.owen_calls) == 1 and eng.groups_calls == [] and eng.calls == [] and eng.launched == 0
    np.testing.assert_array_equal(eng.owen_calls[0], labels)
    assert res.attribution.shape == (p,) and res.group_attribution.shape == (3,) and res.theta.shape == (p,)
    assert isinstance(res.r_squared, float) and isinstance(res.baseline_r_squared, float)
    prob = gram_problem(*d, reg=0.1)
    np.testing.assert_allclose(res.attribution, owen_values(*prob, labels), rtol=0, atol=1e-13)
    np.testing.assert_array_equal(res.group_attribution, ref.attribution)
    np.testing.assert_array_equal(res.theta, ref.theta)
    assert res.r_squared == ref.r_squared
    assert (res.attribution[labels == -1] == 0.0).all()
    assert abs(res.baseline_r_squared - value(*prob, np.nonzero(labels == -1)[0])) < 1e-13
    for k in range(3):
        assert abs(res.attribution[labels == k].sum() - res.group_attribution[k]) < 1e-13
    assert abs(res.attribution.sum() - (res.r_squared - res.baseline_r_squared)) < 1e-12


def test_no_baseline_has_baseline_r_squared_zero():
    res = ls_spa_owen(*data(5, seed=71), [0, 0, 1, 1, 1], _engine=OwenOracleEngine())
    assert res.baseline_r_squared == 0.0 and abs(res.attribution.sum() - res.r_squared) < 1e-12


def test_kept_engine_back_to_float64():
    class Float32Engine(OwenOracleEngine):
        precision = "float32"

        def set_precision(self, dtype):
            self.precision = np.dtype(dtype).name

        def full_fit(self):
            assert self.precision == "float64", "full fit with fp32 factorisation"
            return super().full_fit()

    eng = Float32Engine()
    ls_spa_owen(*data(6, seed=3), [0, 0, 1, 1, -1, 2], _engine=eng)
    assert eng.precision == "float64"


def test_not_positive_definite_warns():
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        ls_spa_owen(*data(5, seed=2), [0, 0, 1, 1, 1], _engine=OwenOracleEngine(info=1))


# ---- every refusal before any engine -------------------------------------------------------------------------------------
def _no_engine(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("an engine was acquired")
    monkeypatch.setattr(_driver, "_acquire_engine", no_engine)


@pytest.mark.parametrize("p, groups, text", [
    (40, np.minimum(np.arange(40), 32), "at most g = 32"),
    (65, np.arange(65) % 8, "at most p = 64"),
    (60, np.minimum(np.arange(60), 30), "at most 32 players: group 30 has 30 columns beside 30 other groups"),
    (34, np.concatenate([np.zeros(33, dtype=int), [-1]]), "at most 32 players: group 0 has 33 columns"),
    (4, [0, 2, 2, 0], "gap in its numbering.*label 1"),
    (4, [0, 1, 2], "length p = 4"),
    (4, [0, -2, 1, 1], "below -1"),
    (4, [-1, -1, -1, -1], "no group at all"),
    (4, [0.0, 1.0, 1.0, 0.0], "integer labels"),
])
def test_refused_before_any_engine(monkeypatch, p, groups, text):
    _no_engine(monkeypatch)
    with pytest.raises(ValueError, match=text):
        ls_spa_owen(*data(p, n=2 * p + 20, m=p + 20, seed=1), groups)


def test_32_players_are_taken():
    labels = np.concatenate([np.arange(16), np.full(17, 16)])      # 16 other groups and 17 columns: 33 players
    with pytest.raises(ValueError, match="at most 32 players: group 16"):
        _driver.group_labels(labels, 33, max_players=_driver.OWEN_MAX_PLAYERS)
    got, g = _driver.group_labels(labels[:-1], 32, max_players=_driver.OWEN_MAX_PLAYERS)
    assert g == 17 and got.dtype == np.int32 and debug_owen_plan(got)[16]["players"] == 32
